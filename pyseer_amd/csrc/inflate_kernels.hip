// inflate_kernels.hip -- k_bgzf_inflate: the BGZF members of a slab of the k-mer reader, decoded on the device (sh_reader_open_dev under
// SEERHIP_ROUTE kmer_inflate=1, sh_inflate_members_dev).  The decoder is shi_inflate of inflate_dev.h, the text sh_inflate_host runs.
//
// One wavefront (a workgroup of 64) per member.  The member's whole output window, 64 KB, lies in LDS with the Huffman tables behind it
// (69 KB of the CU's 160: two workgroups per CU), so a back-reference is an LDS read and no byte of text goes to global memory while the
// member is being decoded.  The compressed bytes are NOT staged: they are read once, front to back, eight bytes per refill of the bit
// buffer, every lane the same address (one request per refill).  Staging them whole would cost up to 64 KB more LDS and leave one
// wavefront on a CU; passing them through a 2 KB window in LDS that the lanes fill 1 KB at a time was built and measured and changed
// nothing (345 ms against 338 ms for 1.5 GB of text, DESIGN 5.5: the wavefront is bound by the instructions it issues per symbol, not
// by the refill's latency), so the plain load stayed.
// All 64 lanes run the decoder on the same values (inflate_dev.h): what is stored once is stored by lane 0, and the lanes share what has a
// byte per step -- clearing the lookup tables, stored blocks and the copies of matches.
// A match of k-mer text is tens of bytes (a sample name and its separator, a k-mer's tail), and one lane copying it through LDS pays one
// round trip per byte.
//
// At the end the lanes copy min(produced, isize) bytes of the window to text + ooff, and this is the only store to the text there is: a
// write outside the member's range cannot happen, whatever the decoder met.  The window begins (text + ooff) mod 16 bytes into its LDS
// array, so LDS and global addresses agree modulo 16 and the body of the copy is whole, aligned 16-byte stores (1 KB per step of the
// wavefront); the bytes before the first and behind the last aligned address go one per lane.
#include "common.h"
#include "inflate_dev.h"

#define INFL_WG 64
#define INFL_WINDOW (SHI_MEMBER_MAX + 16)

struct ShInfWave {
    __device__ uint32_t lane() const { return threadIdx.x; }
    __device__ uint32_t width() const { return INFL_WG; }
    // (LDS operations of one wavefront complete in issue order: nothing to wait for, the compiler must only keep the order)
    __device__ void sync() const { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }
};

__global__ __launch_bounds__(INFL_WG) void k_bgzf_inflate(const uint8_t *__restrict__ comp, const ShInfMember *__restrict__ mem, uint8_t *__restrict__ text,
                                                          int32_t *__restrict__ status, uint32_t *__restrict__ produced)
{
    extern __shared__ uint4 s_infl[];                     // [INFL_WINDOW bytes of window][ShInfTables]
    uint8_t *const win = (uint8_t *)s_infl;
    ShInfTables *const t = (ShInfTables *)(win + INFL_WINDOW);
    const uint32_t lane = threadIdx.x;
    const ShInfMember m = mem[blockIdx.x];
    uint8_t *const dst = text + m.ooff;
    const uint32_t shift = (uint32_t)((uintptr_t)dst & 15u);
    const uint32_t isize = m.isize < SHI_MEMBER_MAX ? m.isize : SHI_MEMBER_MAX;      // (never more than the window holds)
    uint32_t n = 0;
    int st = shi_inflate(comp + m.coff, m.clen, win + shift, isize, t, &n, ShInfWave());
    if (m.isize > SHI_MEMBER_MAX) st = SHI_OUTPUT_FULL;
    if (n > isize) n = isize;
    __syncthreads();
    // window positions [lo, hi) hold the text; position p goes to base + p, and base is a multiple of 16
    uint8_t *const base = dst - shift;
    const uint32_t lo = shift, hi = shift + n;
    const uint32_t a = (lo + 15u) & ~15u, z = hi & ~15u;
    if (a >= z) {
        for (uint32_t p = lo + lane; p < hi; p += INFL_WG) base[p] = win[p];
    } else {
        if (lo + lane < a) base[lo + lane] = win[lo + lane];
        for (uint32_t p = a + lane * 16u; p < z; p += INFL_WG * 16u) *(uint4 *)(base + p) = *(const uint4 *)(win + p);
        if (z + lane < hi) base[z + lane] = win[z + lane];
    }
    if (lane == 0) { status[blockIdx.x] = st; produced[blockIdx.x] = n; }
}

size_t shk_bgzf_inflate_lds_bytes() { return (size_t)INFL_WINDOW + sizeof(ShInfTables); }

hipError_t shk_bgzf_inflate(hipStream_t st, const uint8_t *comp, const ShInfMember *mem, int64_t n, uint8_t *text, int32_t *status, uint32_t *produced)
{
    if (n <= 0) return hipSuccess;
    const size_t lds = shk_bgzf_inflate_lds_bytes();
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_bgzf_inflate), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)n), dim3(INFL_WG), lds, st, comp, mem, text, status, produced);
    return hipGetLastError();
}
