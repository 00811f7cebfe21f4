// patset_kernels.hip -- the run-wide set of distinct presence patterns (--count-patterns).
//
// The reference finds the number of distinct patterns of a run in two steps: --output-patterns writes base64(md5) of every tested variant
// (pyseer/input.py:710-723), scripts/count_patterns.py runs `sort -u | wc -l` over that file.  Here the set lives in HBM across the blocks of
// a run: an open-addressing table of 128-bit keys (patset_hash.h; or the 16 digest bytes of a host-made md5), linear probing from
// key[0] & (slots - 1), two 64-bit arrays k1 / k2 that start as PS_EMPTY.
//
// Insert without a 128-bit compare-and-swap and without any lane waiting for another: at slot s
//     prev = CAS(k1[s], EMPTY, a)      prev neither EMPTY nor a       -> next slot
//     p2   = CAS(k2[s], EMPTY, b)      p2 == EMPTY: the key is NEW;  p2 == b: it was there;  else (same first half, other key) -> next slot
// A word, once set, never changes, so every decision depends on a slot's FINAL contents only: two threads with one key walk the same
// slots, stop at the same one, and exactly one of them sees EMPTY on k2.  Whoever matches the first half may publish the second.  Before
// any atomic both words are read with plain loads (a stale EMPTY only sends the lane to the atomic): most rows of real data repeat patterns
// of earlier blocks.  The probe loop is bounded by the capacity and sets cnt[1] when it gives up (the host keeps the load <= 1/2 and checks
// the word: patset_api.inc).
#include "common.h"
#include "patset_hash.h"

// -> 1 the key is new, 0 it was present (or the table is full: cnt[1] set)
__device__ __forceinline__ int ps_insert(unsigned long long *__restrict__ k1, unsigned long long *__restrict__ k2, uint64_t mask, uint64_t a, uint64_t b,
                                         unsigned long long *__restrict__ cnt)
{
    a = ps_remap(a); b = ps_remap(b);
    uint64_t s = a & mask;
    for (uint64_t probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {
        uint64_t x = k1[s], y = k2[s];
        if (x == a && y == b) return 0;
        if (x == PS_EMPTY) { x = atomicCAS(&k1[s], (unsigned long long)PS_EMPTY, (unsigned long long)a); if (x == PS_EMPTY) x = a; }
        if (x != a) continue;
        if (y == PS_EMPTY) {
            y = atomicCAS(&k2[s], (unsigned long long)PS_EMPTY, (unsigned long long)b);
            if (y == PS_EMPTY) return 1;
        }
        if (y == b) return 0;
    }
    atomicOr(&cnt[1], 1ull);
    return 0;
}

// one add per wavefront to the count of distinct keys
__device__ __forceinline__ void ps_count(bool is_new, unsigned long long *__restrict__ cnt)
{
    const unsigned long long m = __ballot(is_new);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt[0], (unsigned long long)__popcll(m));
}

// Rows as submitted (row-major, row_bytes each): one wavefront hashes a row, 64 rows in turn, lane r keeps the key of row r; then the 64
// lanes insert side by side.  flags (or null): rows with SH_FLAG_PREFILTER are not part of the set (never tested).
__global__ __launch_bounds__(256) void k_ps_insert_rows(const uint8_t *__restrict__ bits, int64_t row_bytes, int64_t V, int N,
                                                        const uint32_t *__restrict__ flags, unsigned long long *__restrict__ k1,
                                                        unsigned long long *__restrict__ k2, uint64_t mask, unsigned long long *__restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    const int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (base >= V) return;                                          // (the whole wavefront)
    const int nr = (int)(V - base < 64 ? V - base : 64), nw = (N + 63) >> 6;
    const bool aligned = (row_bytes & 7) == 0 && ((uintptr_t)bits & 7) == 0;
    const unsigned long long skip = __ballot(flags != nullptr && lane < nr && (flags[base + (lane < nr ? lane : 0)] & SH_FLAG_PREFILTER) != 0);
    uint64_t ka = 0, kb = 0; bool have = false;
#pragma unroll 4
    for (int r = 0; r < nr; ++r) {
        if ((skip >> r) & 1ull) continue;
        const uint8_t *row = bits + (base + r) * row_bytes;
        uint64_t a = 0, b = 0;
        for (int i = lane; i < nw; i += 64) {
            const uint64_t w = ps_row_word(row, row_bytes, N, i, aligned);
            a += ps_word0(w, (uint64_t)i); b += ps_word1(w, (uint64_t)i);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { a += __shfl_xor((unsigned long long)a, o); b += __shfl_xor((unsigned long long)b, o); }
        if (lane == r) { ka = ps_fin0(a); kb = ps_fin1(b); have = true; }
    }
    const int is_new = have ? ps_insert(k1, k2, mask, ka, kb, cnt) : 0;
    ps_count(is_new != 0, cnt);
}

// keys made elsewhere (two words each): one lane per key
__global__ __launch_bounds__(256) void k_ps_insert_keys(const uint64_t *__restrict__ keys, int64_t n, unsigned long long *__restrict__ k1,
                                                        unsigned long long *__restrict__ k2, uint64_t mask, unsigned long long *__restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int is_new = i < n ? ps_insert(k1, k2, mask, keys[2 * i], keys[2 * i + 1], cnt) : 0;
    ps_count(is_new != 0, cnt);
}

// md5 digests made on the device (the job stream's call blocks: k_job_md5_calls), four words per row: the rows that are tested (no
// SH_FLAG_PREFILTER) and hold a missing call enter as their digest, as sh_patset_add_keys takes the host's digests; one lane per row
__global__ __launch_bounds__(256) void k_ps_insert_digests(const uint32_t *__restrict__ digest, int64_t V, const uint32_t *__restrict__ flags,
                                                           const int32_t *__restrict__ n_missing, unsigned long long *__restrict__ k1,
                                                           unsigned long long *__restrict__ k2, uint64_t mask, unsigned long long *__restrict__ cnt)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int is_new = 0;
    if (v < V && !(flags[v] & SH_FLAG_PREFILTER) && n_missing[v] != 0) {
        const uint32_t *d = digest + (size_t)v * 4;
        is_new = ps_insert(k1, k2, mask, (uint64_t)d[0] | ((uint64_t)d[1] << 32), (uint64_t)d[2] | ((uint64_t)d[3] << 32), cnt);
    }
    ps_count(is_new != 0, cnt);
}

// growth: the stored pairs of the old table into the new one (the count does not move: every pair is distinct)
__global__ __launch_bounds__(256) void k_ps_rehash(const unsigned long long *__restrict__ o1, const unsigned long long *__restrict__ o2, int64_t old_slots,
                                                   unsigned long long *__restrict__ k1, unsigned long long *__restrict__ k2, uint64_t mask,
                                                   unsigned long long *__restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= old_slots) return;
    const uint64_t a = o1[i], b = o2[i];
    if (a == PS_EMPTY || b == PS_EMPTY) return;
    (void)ps_insert(k1, k2, mask, a, b, cnt);
}

extern "C" {

hipError_t shk_ps_insert_rows(hipStream_t st, const uint8_t *bits, int64_t row_bytes, int64_t V, int N, const uint32_t *flags,
                              unsigned long long *k1, unsigned long long *k2, int64_t slots, unsigned long long *cnt)
{
    if (V <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ps_insert_rows, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, st, bits, row_bytes, V, N, flags, k1, k2, (uint64_t)(slots - 1), cnt);
    return hipGetLastError();
}

hipError_t shk_ps_insert_keys(hipStream_t st, const uint64_t *keys, int64_t n, unsigned long long *k1, unsigned long long *k2, int64_t slots,
                              unsigned long long *cnt)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ps_insert_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keys, n, k1, k2, (uint64_t)(slots - 1), cnt);
    return hipGetLastError();
}

hipError_t shk_ps_insert_digests(hipStream_t st, const uint32_t *digest, int64_t V, const uint32_t *flags, const int32_t *n_missing, unsigned long long *k1,
                                 unsigned long long *k2, int64_t slots, unsigned long long *cnt)
{
    if (V <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ps_insert_digests, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, st, digest, V, flags, n_missing, k1, k2, (uint64_t)(slots - 1), cnt);
    return hipGetLastError();
}

hipError_t shk_ps_rehash(hipStream_t st, const unsigned long long *o1, const unsigned long long *o2, int64_t old_slots, unsigned long long *k1,
                         unsigned long long *k2, int64_t slots, unsigned long long *cnt)
{
    hipLaunchKernelGGL(k_ps_rehash, dim3((unsigned)((old_slots + 255) / 256)), dim3(256), 0, st, o1, o2, old_slots, k1, k2, (uint64_t)(slots - 1), cnt);
    return hipGetLastError();
}

}  // extern "C"
