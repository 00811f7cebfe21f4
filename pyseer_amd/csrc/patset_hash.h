// patset_hash.h -- the 128-bit key of a packed presence row, one definition for the host (sh_patset_hash_rows) and the device
// (patset_kernels.hip).
//
// Two rows get the same md5 from the reference's hash_pattern (pyseer/input.py:710-723) exactly when their N sample bits are equal, so the
// number of distinct patterns of a run (scripts/count_patterns.py: `sort -u | wc -l` over the md5 lines) is the number of distinct packed
// rows.  The key is two independently seeded 64-bit sums over the row's 64-bit words:
//     half_s = fin_s( sum over words i of word_s(w_i, i) )        s = 0, 1
// word_s is a bijection of w for every (s, i) -- rows that differ in one word always differ in both halves -- and depends on the word's
// index, so equal words at different places do not cancel.  The sum is commutative: the lanes of a wavefront add their words' terms in any
// order (a butterfly of __shfl_xor) and the host adds them front to back, with the same result.  Only the N sample bits enter: the ragged
// last word is masked, bytes past row_bytes count as zero.  With n distinct rows the chance of any two sharing a key is about n^2 / 2^129,
// the order of md5's own.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define PS_EMPTY 0xFFFFFFFFFFFFFFFFull          // the table's empty marker; a key half that equals it is stored as 0 (ps_remap)

__host__ __device__ inline uint64_t ps_word0(uint64_t w, uint64_t i)
{
    uint64_t x = w ^ (0x243F6A8885A308D3ull + (i + 1) * 0x9E3779B97F4A7C15ull);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}

__host__ __device__ inline uint64_t ps_word1(uint64_t w, uint64_t i)
{
    uint64_t x = w ^ (0x13198A2E03707344ull + (i + 1) * 0xC2B2AE3D27D4EB4Full);
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 29;
    return x;
}

__host__ __device__ inline uint64_t ps_fin0(uint64_t x) { x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 32; return x; }
__host__ __device__ inline uint64_t ps_fin1(uint64_t x) { x ^= x >> 29; x *= 0x9FB21C651E98DF25ull; x ^= x >> 32; return x; }

// A half equal to the marker is stored as 0: the keys (~0, b) and (0, b) count as one, and so do (a, ~0) and (a, 0).  For a hashed row or
// an md5 digest that is a 2^-64 event per half.
__host__ __device__ inline uint64_t ps_remap(uint64_t h) { return h == PS_EMPTY ? 0ull : h; }

// word i of a row of row_bytes bytes (little-endian), bytes past the row's end zero, bits from sample N on cleared
__host__ __device__ inline uint64_t ps_row_word(const uint8_t *row, int64_t row_bytes, int N, int i, bool aligned)
{
    uint64_t x = 0;
    if (aligned) x = reinterpret_cast<const uint64_t *>(row)[i];
    else for (int b = 0; b < 8 && (int64_t)i * 8 + b < row_bytes; ++b) x |= (uint64_t)row[(int64_t)i * 8 + b] << (8 * b);
    if (i == ((N + 63) >> 6) - 1 && (N & 63)) x &= (1ull << (N & 63)) - 1ull;
    return x;
}
