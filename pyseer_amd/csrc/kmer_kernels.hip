// kmer_kernels.hip -- the device half of the k-mer reader's device route (sh_reader_open_dev): "KMER | sample:count sample:count ..." lines,
// as the decoder wrote them into the reader's slabs, to packed presence rows.  The rule is stated once in kmer_kernels.h (host_kmer_pack).
//
// k_kmer_pack: one workgroup of 256 per line, the row in LDS.  The line lies somewhere in the device copy of a slab; the lanes take it in
// chunks of 16 bytes at addresses that are multiples of 16 (one dwordx4 each; the chunk that holds the line's first or last byte also holds
// bytes that are not the line's, which are masked by position -- the copy has KMER_SLACK bytes behind it, so every such chunk lies inside
// the allocation), a step of the workgroup being 4 KB.
//   pass 1  every '|' of the line: each lane keeps the first two of its chunks; the smallest of all is the first bar (LDS atomicMin), the
//           smallest behind it the second.  The segment is what lies between them, or up to the line's end.
//   pass 2  a byte of the segment that is no blank and follows a blank (or opens the segment) is a token's first byte, and the token belongs
//           to the lane whose chunk holds it.  That lane walks on from there -- out of its chunk if need be, byte loads from the cached line
//           -- to the first ':' or blank, hashing as it goes, looks the name up, compares length and bytes, and sets the sample's bit with
//           an LDS atomicOr.
//   the row leaves as whole words, the count is its popcount.
// The line is read twice; the second time it comes from the cache (a line at N = 5000 is 37 KB).
#include "common.h"
#include "kmer_kernels.h"

#define KMER_WG 256

__global__ __launch_bounds__(256) void k_kmer_table_build(int32_t *__restrict__ slot, const uint32_t mask, const uint32_t *__restrict__ name_off,
                                                          const uint32_t *__restrict__ name_len, const uint8_t *__restrict__ blob, const int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t len = name_len[i];
    const uint8_t *me = blob + name_off[i];
    uint32_t h = KMER_HASH_INIT;
    for (uint32_t j = 0; j < len; ++j) h = shk_kmer_hash_step(h, me[j]);
    // a slot, once taken, holds the same NAME for good (only a smaller index of that name replaces its index), so every sample of a name
    // walks past the same slots and stops at the same one
    for (uint32_t k = h & mask, tries = 0; tries <= mask; k = (k + 1) & mask, ++tries) {
        int32_t j = atomicCAS(&slot[k], -1, i);
        if (j == -1) return;
        if (name_len[j] == len) {
            const uint8_t *c = blob + name_off[j];
            uint32_t q = 0;
            while (q < len && c[q] == me[q]) ++q;
            if (q == len) { atomicMin(&slot[k], i); return; }       // the first occurrence wins
        }
    }
}

__global__ __launch_bounds__(KMER_WG) void k_kmer_pack(const uint64_t *__restrict__ bases, const ShKmerRec *__restrict__ recs, const ShKmerTable t,
                                                       const int row_words, uint32_t *__restrict__ rows, int32_t *__restrict__ counts)
{
    extern __shared__ uint32_t s_row[];                   // [row_words]
    __shared__ uint32_t s_bar[2];
    __shared__ int s_cnt;
    const int tid = threadIdx.x;
    const ShKmerRec r = recs[blockIdx.x];
    const uint8_t *__restrict__ buf = (const uint8_t *)bases[r.slab];
    const uint32_t len = r.len, NONE = 0xffffffffu;
    for (int i = tid; i < row_words; i += KMER_WG) s_row[i] = 0;
    if (tid < 2) s_bar[tid] = NONE;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    // Positions are counted from the start of the chunk that holds the line's first byte: the line is [lead, stop) there, and chunk c the
    // bytes [16 c, 16 c + 16).
    const uint32_t lead = r.off & (KMER_LANE_BYTES - 1), stop = lead + len;
    const uint8_t *__restrict__ text = buf + (r.off - lead);
    const uint32_t n_chunks = (stop + KMER_LANE_BYTES - 1) / KMER_LANE_BYTES;
    // ---- pass 1: the bars
    uint32_t p1 = NONE, p2 = NONE;
    for (uint32_t c = tid; c < n_chunks; c += KMER_WG) {
        const uint4 v = *(const uint4 *)(text + (size_t)c * KMER_LANE_BYTES);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < KMER_LANE_BYTES; ++j) {
            const uint32_t pos = c * KMER_LANE_BYTES + (uint32_t)j;
            if (((w[j >> 2] >> (8 * (j & 3))) & 0xffu) == '|' && pos >= lead && pos < stop) { if (p1 == NONE) p1 = pos; else if (p2 == NONE) p2 = pos; }
        }
    }
    if (p1 != NONE) atomicMin(&s_bar[0], p1);
    __syncthreads();
    const uint32_t bar = s_bar[0];
    const uint32_t cand = (p1 != NONE && p1 > bar) ? p1 : p2;       // (p1 < bar cannot be; p1 == bar: my next one)
    if (cand != NONE) atomicMin(&s_bar[1], cand);
    __syncthreads();
    // ---- pass 2: the tokens of [seg, end)
    if (bar != NONE) {
        const uint32_t seg = bar + 1, end = min(s_bar[1], stop);
        const uint32_t c_from = seg / KMER_LANE_BYTES, c_to = (end + KMER_LANE_BYTES - 1) / KMER_LANE_BYTES;
        for (uint32_t c = c_from + tid; c < c_to; c += KMER_WG) {
            const uint4 v = *(const uint4 *)(text + (size_t)c * KMER_LANE_BYTES);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const uint32_t first = c * KMER_LANE_BYTES;                          // position of my byte 0
            uint32_t blank = 0, inside = 0;
#pragma unroll
            for (int j = 0; j < KMER_LANE_BYTES; ++j) {
                const uint32_t pos = first + (uint32_t)j;
                if (shk_kmer_blank((w[j >> 2] >> (8 * (j & 3))) & 0xffu)) blank |= 1u << j;
                if (pos >= seg && pos < end) inside |= 1u << j;
            }
            // the byte before my chunk counts as a blank where it is not the segment's; the segment's first byte opens a token if it is no blank
            uint32_t prev_blank = (blank << 1) | ((first > seg && shk_kmer_blank(text[first - 1])) ? 1u : 0u);
            if (seg >= first) prev_blank |= 1u << (seg - first);                 // (seg - first < 16: c >= c_from)
            uint32_t starts = ~blank & prev_blank & inside & 0xffffu;
            while (starts) {
                const uint32_t j = (uint32_t)__ffs((int)starts) - 1u;
                starts &= starts - 1u;
                const uint32_t p = first + j;
                uint32_t q = p, h = KMER_HASH_INIT;
                while (q < end) {
                    const uint32_t ch = text[q];
                    if (shk_kmer_blank(ch) || ch == ':') break;
                    h = shk_kmer_hash_step(h, ch);
                    ++q;
                }
                const int i = shk_kmer_find(t, text + p, q - p, h);
                if (i >= 0) atomicOr(&s_row[i >> 5], 1u << (i & 31));
            }
        }
    }
    __syncthreads();
    int n = 0;
    uint32_t *__restrict__ out = rows + (size_t)r.row * (size_t)row_words;
    for (int i = tid; i < row_words; i += KMER_WG) { const uint32_t x = s_row[i]; out[i] = x; n += __popc(x); }
    if (n) atomicAdd(&s_cnt, n);
    __syncthreads();
    if (tid == 0) counts[r.row] = s_cnt;
}

size_t shk_kmer_lds_bytes(int row_words) { return (size_t)row_words * 4; }

hipError_t shk_kmer_table_build(hipStream_t st, int32_t *slot, uint32_t mask, const uint32_t *name_off, const uint32_t *name_len, const uint8_t *blob, int n)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_kmer_table_build, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, slot, mask, name_off, name_len, blob, n);
    return hipGetLastError();
}

hipError_t shk_kmer_pack(hipStream_t st, const uint64_t *bases, const ShKmerRec *recs, int64_t n_lines, ShKmerTable table, int row_words,
                         uint32_t *rows, int32_t *counts)
{
    if (n_lines <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_kmer_pack, dim3((unsigned)n_lines), dim3(KMER_WG), shk_kmer_lds_bytes(row_words), st, bases, recs, table, row_words, rows, counts);
    return hipGetLastError();
}
