// simtext_kernels.hip -- the similarity matrix as the text the reference prints (pyseer/similarity.py:116:
// pd.DataFrame(K, index=names, columns=names).to_csv(sep='\t')), made where K is: on the device.
//
//   header   ""  then  \t name_j  for every sample,  \n
//   row i    name_i  then  \t cell_ij  for every sample,  \n
//   cell     the count's decimal digits and ".0" (what repr() makes of an integer-valued double below 1e16); empty where sample i or j is
//            flagged in nan_mask (the NaN rows and columns of a matrix with missing calls).
//
// Two passes over K, one workgroup of 256 threads per matrix row in each:
//   k_sim_text_len   every cell's length, reduced to the row's; cells the rule cannot express (non-integers, negatives, >= 1e15) set a bit
//                    of *bad and the caller refuses the matrix;
//   (the caller scans the N row lengths on the host: it needs the total there anyway, for the capacity check)
//   k_sim_format     256 cells at a time: a block-wide exclusive scan of the cell lengths places each cell, its characters go to LDS at the
//                    position they will have in global memory modulo 16, and the chunk leaves in 16-byte stores (bytes at its two ragged ends).
//                    Block N writes the header.
// All offsets into the text are 64-bit (N = 20 000: 4 GB).
#include <hip/hip_runtime.h>
#include <cstdint>

#define ST_THREADS 256
#define ST_CELL_MAX 18              // \t + 15 digits + ".0"
#define ST_BAD_FRACTION 1u
#define ST_BAD_NEGATIVE 2u
#define ST_BAD_LARGE 4u

// digits of v < 1e15
__device__ __forceinline__ int st_ndigits(uint64_t v)
{
    int n = 1;
    uint64_t p = 10;
    while (v >= p) { ++n; p *= 10; }          // (p ends at 1e15 at most: no overflow)
    return n;
}

// the cell's length with its leading tab; *v the count (0 for an empty cell); bad: the cases met
__device__ __forceinline__ int st_cell(double x, bool empty, uint64_t *v, unsigned *bad)
{
    *v = 0;
    if (empty) return 1;
    if (!(x >= 0.0) || __builtin_signbit(x)) { *bad |= (x != x) ? ST_BAD_FRACTION : ST_BAD_NEGATIVE; return 1; }
    if (x >= 1e15) { *bad |= ST_BAD_LARGE; return 1; }
    const uint64_t u = (uint64_t)x;
    if ((double)u != x) { *bad |= ST_BAD_FRACTION; return 1; }
    *v = u;
    return 3 + st_ndigits(u);
}

// exclusive scan of one int per thread over the 256 threads; *total the block's sum.  wsum: 4 ints of LDS; two barriers.
__device__ __forceinline__ int st_block_scan(int x, int *wsum, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(incl, d, 64); if (lane >= d) incl += y; }
    __syncthreads();                               // (the previous round's wsum has been read)
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < ST_THREADS / 64; ++w) { const int s = wsum[w]; if (w < wave) base += s; all += s; }
    *total = all;
    return base + incl - x;
}

__global__ __launch_bounds__(ST_THREADS) void k_sim_text_len(const double *__restrict__ K, int N, const int64_t *__restrict__ names_off,
                                                             const uint8_t *__restrict__ nan_mask, int64_t *__restrict__ row_len,
                                                             unsigned *__restrict__ bad)
{
    __shared__ int wsum[ST_THREADS / 64];
    const int i = blockIdx.x;
    const bool row_empty = nan_mask && nan_mask[i];
    const double *row = K + (int64_t)i * N;
    int len = 0;
    unsigned b = 0;
    for (int j = threadIdx.x; j < N; j += ST_THREADS) {
        uint64_t v;
        len += st_cell(row[j], row_empty || (nan_mask && nan_mask[j]), &v, &b);
    }
    int total;
    st_block_scan(len, wsum, &total);              // (a row of 2^19 cells of 18 bytes is below 2^31)
    if (threadIdx.x == 0) row_len[i] = (names_off[i + 1] - names_off[i]) + (int64_t)total + 1;
    if (b) atomicOr(bad, b);
}

__global__ __launch_bounds__(ST_THREADS) void k_sim_format(const double *__restrict__ K, int N, const char *__restrict__ names,
                                                           const int64_t *__restrict__ names_off, const uint8_t *__restrict__ nan_mask,
                                                           const int64_t *__restrict__ row_off, uint8_t *__restrict__ out)
{
    __shared__ int wsum[ST_THREADS / 64];
    __shared__ __attribute__((aligned(16))) uint8_t buf[ST_THREADS * ST_CELL_MAX + 32];
    const int tid = threadIdx.x;
    const int64_t n0 = names_off[0];
    if ((int)blockIdx.x == N) {                    // the header: name j follows its tab at (names_off[j] - n0) + j
        for (int j = tid; j < N; j += ST_THREADS) {
            const int64_t a = names_off[j], e = names_off[j + 1];
            uint8_t *o = out + (a - n0) + j;
            *o++ = '\t';
            for (int64_t k = a; k < e; ++k) *o++ = (uint8_t)names[k];
        }
        if (tid == 0) out[(names_off[N] - n0) + N] = '\n';
        return;
    }
    const int i = blockIdx.x;
    const bool row_empty = nan_mask && nan_mask[i];
    const double *row = K + (int64_t)i * N;
    int64_t g = row_off[i];
    {
        const int64_t a = names_off[i], e = names_off[i + 1];
        for (int64_t k = a + tid; k < e; k += ST_THREADS) out[g + (k - a)] = (uint8_t)names[k];
        g += e - a;
    }
    for (int j0 = 0; j0 < N; j0 += ST_THREADS) {
        const int j = j0 + tid;
        uint64_t v = 0;
        unsigned b = 0;
        int len = 0;
        if (j < N) len = st_cell(row[j], row_empty || (nan_mask && nan_mask[j]), &v, &b);
        int total;
        const int at = st_block_scan(len, wsum, &total);
        const int shift = (int)(g & 15);           // buf[shift + k] is the text's byte g + k: LDS and global memory agree modulo 16
        if (len) {
            uint8_t *o = buf + shift + at;
            o[0] = '\t';
            if (len > 1) {
                o[len - 1] = '0'; o[len - 2] = '.';
                for (int k = len - 3; k >= 1; --k) { const uint64_t q = v / 10; o[k] = (uint8_t)('0' + (int)(v - q * 10)); v = q; }
            }
        }
        __syncthreads();
        // 16-byte segments of [g - shift, g + total): whole ones as one store, the ragged first and last by bytes
        const int nseg = (shift + total + 15) >> 4;
        uint8_t *o16 = out + (g - shift);
        for (int s = tid; s < nseg; s += ST_THREADS) {
            const int lo = s << 4;
            if (lo >= shift && lo + 16 <= shift + total) {
                *reinterpret_cast<uint4 *>(o16 + lo) = *reinterpret_cast<const uint4 *>(buf + lo);
            } else {
                const int k0 = lo > shift ? lo : shift, k1 = lo + 16 < shift + total ? lo + 16 : shift + total;
                for (int k = k0; k < k1; ++k) o16[k] = buf[k];
            }
        }
        g += total;
        __syncthreads();                           // (buf is written again)
    }
    if (tid == 0) out[g] = '\n';
}

extern "C" {

// row_len[i] = bytes of line i + 1 (the line of sample i); *bad |= the ST_BAD_* cases met.  K: N x N on the device.
hipError_t shk_sim_text_len(hipStream_t st, const double *K, int N, const int64_t *names_off, const uint8_t *nan_mask, int64_t *row_len, unsigned *bad)
{
    hipLaunchKernelGGL(k_sim_text_len, dim3((unsigned)N), dim3(ST_THREADS), 0, st, K, N, names_off, nan_mask, row_len, bad);
    return hipGetLastError();
}

// out: the whole text (16-byte aligned); row_off[i]: where the line of sample i begins (the header's length + the lines before it)
hipError_t shk_sim_format(hipStream_t st, const double *K, int N, const char *names, const int64_t *names_off, const uint8_t *nan_mask,
                          const int64_t *row_off, uint8_t *out)
{
    if ((uintptr_t)out & 15) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sim_format, dim3((unsigned)N + 1), dim3(ST_THREADS), 0, st, K, N, names, names_off, nan_mask, row_off, out);
    return hipGetLastError();
}

}  // extern "C"
