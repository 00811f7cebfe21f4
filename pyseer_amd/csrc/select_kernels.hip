// select_kernels.hip -- a packed cache served to a subset or another order of its samples: the rows of a block over n_src samples become rows
// over n_dst of them, bit j of a new row = bit map[j] of the old one.
//
// k_rows_select<R>: one wavefront per R consecutive rows, blockDim.x / 64 wavefronts per workgroup.
//   * the wavefront's R source rows are contiguous in memory: they go to the wavefront's own part of the LDS as they stand, 8 bytes per lane
//     and step (rows are 8-byte aligned: row_bytes_for), pad bits included -- nothing below reads them, since every map entry is < n_src;
//   * step w makes output word w (64 bits) of all R rows: lane l loads map[64 w + l] once (coalesced; the table is shared by every row and
//     stays in the caches) and picks that bit of each of the R rows from the LDS; a ballot per row is the output word, which lane w & 63
//     keeps in a register; lanes with 64 w + l >= n_dst vote 0, so the pad bits of the ragged last word are zeros;
//   * after 64 steps, and after the last, the kept words leave with one coalesced 8-byte store per lane and row;
//   * a row's count is the sum of the popcounts of its ballots.
// R = 4 shares a map load between four rows (the table is 4 n_dst bytes against n_src / 8 of a row: with one row per wavefront the table
// is 30 times the row's own traffic); a source row too wide for sixteen rows per workgroup in 64 KB of LDS takes R = 1 with four
// wavefronts, then one wavefront; wider than 64 KB is refused by the caller (shk_rows_select_max_row_bytes).
// All stores are plain vector stores; the map is validated by the host (csrc/select_api.inc) before it is uploaded.
//
// k_calls_select<R>: the same pass over a block of CALLS (a call cache: DESIGN.md section 5.9) -- a present and a missing plane of the same
// rows.  The wavefront stages its R rows of BOTH planes, [plane][R][src_words], and step w loads map[64 w + l] once for the 2 R ballots it
// makes: the output words of present' and missing', whose popcounts are n_present' and n_missing'.  The same 64 KB of LDS now hold half
// as many rows: R = 4 with 4, 2 or 1 wavefronts while 8 source rows of a wavefront fit (src_row_bytes <= 2048, 4096, 8192 -- the map load
// stays shared by eight ballots; a lone wavefront with 64 KB leaves a CU two wavefronts, which only a run over 32 768 samples and more
// meets), then R = 1 with 2 or 1 wavefronts (<= 16 384, 32 768); a wider source row does not fit one wavefront's two planes and is refused
// by the caller (shk_calls_select_max_row_bytes).
#include "common.h"

#define SELECT_LDS_MAX 65536

template <int R>
__global__ __launch_bounds__(256) void k_rows_select(const uint64_t *__restrict__ src, const int src_words, const int64_t V, const int32_t *__restrict__ map,
                                                     const int n_dst, const int out_words, uint64_t *__restrict__ out, int32_t *__restrict__ counts)
{
    extern __shared__ uint64_t s_sel[];                   // [wavefronts][R][src_words]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int64_t row0 = ((int64_t)blockIdx.x * waves + wave) * R;
    const int nr = row0 < V ? (int)min((int64_t)R, V - row0) : 0;      // rows of this wavefront (0: a wavefront behind the last row)
    uint64_t *mine = s_sel + (size_t)wave * R * src_words;
    const uint64_t *from = src + (size_t)row0 * src_words;
    for (int i = lane; i < nr * src_words; i += 64) mine[i] = from[i];
    __syncthreads();
    if (nr == 0) return;
    const uint32_t *m32 = (const uint32_t *)mine;         // (little-endian: bit m of a row is bit m & 31 of its 32-bit word m >> 5)
    uint64_t keep[R];
    int cnt[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { keep[r] = 0; cnt[r] = 0; }
    for (int w = 0; w < out_words; ++w) {
        const int j = 64 * w + lane;
        const bool in = j < n_dst;
        const int m = in ? map[j] : 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            // (a row at or behind nr was not staged: what it reads lies inside the wavefront's own LDS and is never stored)
            const uint32_t word = m32[(size_t)r * src_words * 2 + (m >> 5)];
            const unsigned long long b = __ballot(in && ((word >> (m & 31)) & 1u));
            cnt[r] += __popcll(b);
            if (lane == (w & 63)) keep[r] = b;
        }
        if ((w & 63) == 63 || w == out_words - 1) {
            const int base = w & ~63;
            if (base + lane <= w) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (r < nr) out[(size_t)(row0 + r) * out_words + base + lane] = keep[r];
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r < nr) counts[row0 + r] = cnt[r];
    }
}

template <int R>
__global__ __launch_bounds__(256) void k_calls_select(const uint64_t *__restrict__ src_p, const uint64_t *__restrict__ src_m, const int src_words, const int64_t V,
                                                      const int32_t *__restrict__ map, const int n_dst, const int out_words, uint64_t *__restrict__ out_p,
                                                      uint64_t *__restrict__ out_m, int32_t *__restrict__ n_p, int32_t *__restrict__ n_m)
{
    extern __shared__ uint64_t s_sel[];                   // [wavefronts][2][R][src_words]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int64_t row0 = ((int64_t)blockIdx.x * waves + wave) * R;
    const int nr = row0 < V ? (int)min((int64_t)R, V - row0) : 0;      // rows of this wavefront (0: a wavefront behind the last row)
    uint64_t *mine_p = s_sel + (size_t)wave * 2 * R * src_words, *mine_m = mine_p + (size_t)R * src_words;
    const uint64_t *from_p = src_p + (size_t)row0 * src_words, *from_m = src_m + (size_t)row0 * src_words;
    for (int i = lane; i < nr * src_words; i += 64) { mine_p[i] = from_p[i]; mine_m[i] = from_m[i]; }
    __syncthreads();
    if (nr == 0) return;
    const uint32_t *p32 = (const uint32_t *)mine_p, *m32 = (const uint32_t *)mine_m;
    uint64_t keep_p[R], keep_m[R];
    int cnt_p[R], cnt_m[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { keep_p[r] = keep_m[r] = 0; cnt_p[r] = cnt_m[r] = 0; }
    for (int w = 0; w < out_words; ++w) {
        const int j = 64 * w + lane;
        const bool in = j < n_dst;
        const int m = in ? map[j] : 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            // (a row at or behind nr was not staged: what it reads lies inside the wavefront's own LDS and is never stored)
            const size_t at = (size_t)r * src_words * 2 + (m >> 5);
            const unsigned long long bp = __ballot(in && ((p32[at] >> (m & 31)) & 1u));
            const unsigned long long bm = __ballot(in && ((m32[at] >> (m & 31)) & 1u));
            cnt_p[r] += __popcll(bp); cnt_m[r] += __popcll(bm);
            if (lane == (w & 63)) { keep_p[r] = bp; keep_m[r] = bm; }
        }
        if ((w & 63) == 63 || w == out_words - 1) {
            const int base = w & ~63;
            if (base + lane <= w) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (r < nr) {
                        out_p[(size_t)(row0 + r) * out_words + base + lane] = keep_p[r];
                        out_m[(size_t)(row0 + r) * out_words + base + lane] = keep_m[r];
                    }
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r < nr) { n_p[row0 + r] = cnt_p[r]; n_m[row0 + r] = cnt_m[r]; }
    }
}

extern "C" {

int64_t shk_rows_select_max_row_bytes(void) { return SELECT_LDS_MAX; }

// src: V rows of src_row_bytes (a multiple of 8, at most shk_rows_select_max_row_bytes()), 8-byte aligned; map: n_dst entries, each below
// src_row_bytes * 8; out: V rows of ((n_dst + 63) / 64) * 8 bytes; counts: V entries
hipError_t shk_rows_select(hipStream_t st, const void *src, int64_t src_row_bytes, int64_t V, const int32_t *map, int n_dst, void *out, int32_t *counts)
{
    if (V <= 0) return hipSuccess;
    if (src_row_bytes <= 0 || (src_row_bytes & 7) || src_row_bytes > SELECT_LDS_MAX || n_dst < 1 || (((uintptr_t)src | (uintptr_t)out) & 7)) return hipErrorInvalidValue;
    const int src_words = (int)(src_row_bytes >> 3), out_words = (n_dst + 63) >> 6;
    if (16 * src_row_bytes <= SELECT_LDS_MAX) {
        const int64_t blocks = (V + 15) / 16;
        hipLaunchKernelGGL(k_rows_select<4>, dim3((unsigned)blocks), dim3(256), (size_t)(16 * src_row_bytes), st, (const uint64_t *)src, src_words, V, map, n_dst,
                           out_words, (uint64_t *)out, counts);
    } else {
        const int waves = 4 * src_row_bytes <= SELECT_LDS_MAX ? 4 : 1;
        const int64_t blocks = (V + waves - 1) / waves;
        hipLaunchKernelGGL(k_rows_select<1>, dim3((unsigned)blocks), dim3(64 * waves), (size_t)(waves * src_row_bytes), st, (const uint64_t *)src, src_words, V, map,
                           n_dst, out_words, (uint64_t *)out, counts);
    }
    return hipGetLastError();
}

// The launch shape of k_calls_select at a source width: rows per wavefront and wavefronts per workgroup; 0 rows: too wide.
static void calls_select_shape(int64_t src_row_bytes, int *R, int *waves)
{
    const int64_t per_row = 2 * src_row_bytes;            // both planes
    *R = 0; *waves = 0;
    if (4 * per_row <= SELECT_LDS_MAX) { *R = 4; *waves = 16 * per_row <= SELECT_LDS_MAX ? 4 : (8 * per_row <= SELECT_LDS_MAX ? 2 : 1); }
    else if (per_row <= SELECT_LDS_MAX) { *R = 1; *waves = 2 * per_row <= SELECT_LDS_MAX ? 2 : 1; }
}

int64_t shk_calls_select_max_row_bytes(void) { return SELECT_LDS_MAX / 2; }

// src_p, src_m: V rows of src_row_bytes each (a multiple of 8, at most shk_calls_select_max_row_bytes()), 8-byte aligned; map as for
// shk_rows_select; out_p, out_m: V rows of ((n_dst + 63) / 64) * 8 bytes, 8-byte aligned; n_p, n_m: V entries each
hipError_t shk_calls_select(hipStream_t st, const void *src_p, const void *src_m, int64_t src_row_bytes, int64_t V, const int32_t *map, int n_dst, void *out_p,
                            void *out_m, int32_t *n_p, int32_t *n_m)
{
    if (V <= 0) return hipSuccess;
    if (src_row_bytes <= 0 || (src_row_bytes & 7) || n_dst < 1 || (((uintptr_t)src_p | (uintptr_t)src_m | (uintptr_t)out_p | (uintptr_t)out_m) & 7)) return hipErrorInvalidValue;
    int R, waves;
    calls_select_shape(src_row_bytes, &R, &waves);
    if (R == 0) return hipErrorInvalidValue;
    const int src_words = (int)(src_row_bytes >> 3), out_words = (n_dst + 63) >> 6;
    const int64_t per = (int64_t)R * waves, blocks = (V + per - 1) / per;
    const size_t lds = (size_t)(2 * per * src_row_bytes);
    if (R == 4)
        hipLaunchKernelGGL(k_calls_select<4>, dim3((unsigned)blocks), dim3(64 * waves), lds, st, (const uint64_t *)src_p, (const uint64_t *)src_m, src_words, V, map, n_dst,
                           out_words, (uint64_t *)out_p, (uint64_t *)out_m, n_p, n_m);
    else
        hipLaunchKernelGGL(k_calls_select<1>, dim3((unsigned)blocks), dim3(64 * waves), lds, st, (const uint64_t *)src_p, (const uint64_t *)src_m, src_words, V, map, n_dst,
                           out_words, (uint64_t *)out_p, (uint64_t *)out_m, n_p, n_m);
    return hipGetLastError();
}

}  // extern "C"
