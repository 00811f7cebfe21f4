// kmer_kernels.h -- the k-mer line tokeniser of the device route (sh_reader_open_dev): the sample table, the rule in plain C++
// (host_kmer_pack: what a reader without a context and the lines no slab holds go through) and the launchers of kmer_kernels.hip.
//
// The rule (pyseer/input.py:377-388, as csrc/reader.cpp states it for the host parser): the sample segment of a line lies between its first
// '|' and the next one (or the line's end); it is split on space, tab and CR; a token is cut at its first ':'; what is left is looked up
// among the phenotype samples by length and bytes (the empty name included); a sample seen sets its bit once.  A line without '|' sets nothing.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define SHK_HD __host__ __device__
#else
#define SHK_HD
#endif

// Open addressing over the sample indices, keyed by the name bytes: slot[h] = the FIRST sample of that name, or -1.  The names themselves are
// one blob with an offset and a length per sample.  The same view serves the kernel (device pointers) and host_kmer_pack (host pointers).
struct ShKmerTable {
    const int32_t *slot;
    const uint32_t *name_off, *name_len;
    const uint8_t *blob;
    uint32_t mask;             // slots - 1 (a power of two, at least 4 per sample: a probe always ends at an empty slot)
};

// a line for the kernel: where its text lies in the device copy of a slab, and which row it fills
struct ShKmerRec {
    uint32_t off;              // of the line's first byte from the start of the slab's buffer
    uint32_t len;              // bytes, without the newline
    uint32_t slab;             // index into the call's table of buffer addresses
    uint32_t row;              // row of the call it writes
};

#define KMER_LANE_BYTES 16     // a thread's chunk: one dwordx4, at an address that is a multiple of 16
#define KMER_SLACK 32          // bytes behind a slab's device copy, so that the chunk holding a line's last byte lies inside the allocation

static inline SHK_HD bool shk_kmer_blank(uint32_t c) { return c == ' ' || c == '\t' || c == '\r'; }
static inline SHK_HD uint32_t shk_kmer_hash_step(uint32_t h, uint32_t c) { return (h ^ c) * 16777619u; }     // FNV-1a, a byte at a time
#define KMER_HASH_INIT 2166136261u

// the sample called [s, s + n) with FNV-1a value h, or -1
static inline SHK_HD int shk_kmer_find(const ShKmerTable &t, const uint8_t *s, uint32_t n, uint32_t h)
{
    for (uint32_t k = h & t.mask, tries = 0; tries <= t.mask; k = (k + 1) & t.mask, ++tries) {
        const int32_t i = t.slot[k];
        if (i < 0) return -1;
        if (t.name_len[i] != n) continue;
        const uint8_t *c = t.blob + t.name_off[i];
        uint32_t j = 0;
        while (j < n && c[j] == s[j]) ++j;
        if (j == n) return i;
    }
    return -1;
}

// The kernel's rule, a byte at a time: row (row_words words, zeroed here) and the number of carriers of one line.
static inline void host_kmer_pack(const char *line, size_t len, const ShKmerTable &t, uint32_t *row, int row_words, int32_t *count)
{
    const uint8_t *b = (const uint8_t *)line;
    for (int i = 0; i < row_words; ++i) row[i] = 0;
    int32_t cnt = 0;
    size_t bar = 0;
    while (bar < len && b[bar] != '|') ++bar;
    if (bar < len) {
        size_t end = bar + 1;
        while (end < len && b[end] != '|') ++end;
        for (size_t p = bar + 1; p < end; ++p) {
            if (shk_kmer_blank(b[p]) || (p > bar + 1 && !shk_kmer_blank(b[p - 1]))) continue;      // not a token's first byte
            uint32_t h = KMER_HASH_INIT;
            size_t q = p;
            while (q < end && !shk_kmer_blank(b[q]) && b[q] != ':') { h = shk_kmer_hash_step(h, b[q]); ++q; }
            const int i = shk_kmer_find(t, b + p, (uint32_t)(q - p), h);
            if (i >= 0 && !((row[i >> 5] >> (i & 31)) & 1u)) { row[i >> 5] |= 1u << (i & 31); ++cnt; }
        }
    }
    *count = cnt;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
size_t shk_kmer_lds_bytes(int row_words);
// the table on the device: one thread per sample inserts its index (the smallest index of a name stays); slot must hold -1 everywhere
hipError_t shk_kmer_table_build(hipStream_t st, int32_t *slot, uint32_t mask, const uint32_t *name_off, const uint32_t *name_len, const uint8_t *blob, int n);
// one workgroup per record: rows[rec.row * row_words ...], counts[rec.row]
hipError_t shk_kmer_pack(hipStream_t st, const uint64_t *bases, const ShKmerRec *recs, int64_t n_lines, ShKmerTable table, int row_words,
                         uint32_t *rows, int32_t *counts);
#endif
