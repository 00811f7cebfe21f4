// lmm_quadform_wide.inc -- THE hot kernel since round 3: the quadratic form with a 128 x 128 wave tile, ONE wavefront per SIMD, 256 accumulators
// in the accumulator half of the unified register file (a[0:255]): half the LDS fragment reads per MFMA of k_lmm_quadform_i8 (4 ds_read_b128 per
// 16 MFMAs instead of per 8).  Included by lmm_kernels.hip; same stage stream, LDS image, ring and epilogue arithmetic as k_lmm_quadform_i8 (see
// the comments there); block = 512 variants, 4 waves x 128 variants; one limb per block (nl = 1), at least four row tiles (the launcher falls back
// to k_lmm_quadform_i8 otherwise).  The launcher says how many segments run (`nfull`, `nit_last`): see the end of the kernel.
//
// Why inline assembly.  hipcc cannot hold 256 accumulators as C++ values here (its allocator copies all of them to VGPRs at every control-flow
// join: the QF_JT = 4 build of round 1 spilled 187 registers inside the MFMA loop), and with one wavefront per SIMD nothing hides a badly placed
// instruction: measured on this kernel (profiles/r03/wide_kernel_notes.md), a lone wavefront hides TWO single-issue instructions in the 32-cycle
// shadow of a 32x32x32 int8 MFMA and pays 6 - 13 cycles for every further one, whatever it is (VALU, SALU, LDS, wait).  The 8 VALU instructions
// that expand a variant fragment from packed bits use that budget up for every group of four MFMAs, so the stage body is four inline-assembly
// statements (the sub-steps; tools/gen_wide_substeps.py writes lmm_quadform_wide_substeps.inc) in which every instruction has its place:
//   * 16 MFMAs per sub-step, the fragment expansion of the NEXT sub-step in their gaps (two per gap), one s_waitcnt lgkmcnt(0) per sub-step (the
//     four A fragments were requested 3 - 4 groups earlier), the next A fragments requested in groups 0 and 1;
//   * the stage's barrier (s_waitcnt vmcnt + s_barrier) behind the first MFMA of sub-step 0, the six LDS-DMAs (buffer_load ... lds through two raw
//     buffer descriptors: the source of a stage is ONE scalar offset each) behind the first MFMA of a group, a fragment instruction between the
//     M0 write and the load instead of an s_nop;
//   * the ring / DMA cursor book-keeping (17 scalar and vector instructions per stage) one per gap in the light groups of sub-steps 2 and 3, in FIXED
//     scalar registers (s84 .. s99) the compiler never sees: an asm statement's scalar OUTPUT is a divergent value to hipcc and lands in a VGPR;
//   * the accumulators named literally (a[0:255], declared through a clobber list, which also makes the kernel descriptor allocate them); the first
//     sub-step of a segment takes C = 0 (no 256 v_accvgpr_write), the stream is walked as segments { first stage ; stages ; epilogue } so that
//     the common path holds no taken branch but the stage loop's own.
// What the compiler still does: VGPR allocation of the operand fragments, the loops, the epilogue's conversions.  Rules kept
// (cdna_hip_programming.md 5.7): LDS reads and LDS-DMAs counted by hand (lgkmcnt / vmcnt), every asm load destination a tied "+v" operand that no
// compiler instruction touches before the wait inside a later statement; MFMA D -> v_accvgpr_read: the epilogue opens with an LDS round trip and
// s_nop 7; M0 written in the statement that uses it.  Build audit after every edit (tools/audit_wide.sh): no scratch, no compiler-generated
// v_accvgpr_*, no compiler use of s84 .. s99.
#define QW_ALL_AGPRS "a0","a1","a2","a3","a4","a5","a6","a7","a8","a9","a10","a11","a12","a13","a14","a15","a16","a17","a18","a19","a20","a21","a22","a23","a24","a25","a26","a27","a28","a29","a30","a31","a32","a33","a34","a35","a36","a37","a38","a39","a40","a41","a42","a43","a44","a45","a46","a47","a48","a49","a50","a51","a52","a53","a54","a55","a56","a57","a58","a59","a60","a61","a62","a63","a64","a65","a66","a67","a68","a69","a70","a71","a72","a73","a74","a75","a76","a77","a78","a79","a80","a81","a82","a83","a84","a85","a86","a87","a88","a89","a90","a91","a92","a93","a94","a95","a96","a97","a98","a99","a100","a101","a102","a103","a104","a105","a106","a107","a108","a109","a110","a111","a112","a113","a114","a115","a116","a117","a118","a119","a120","a121","a122","a123","a124","a125","a126","a127","a128","a129","a130","a131","a132","a133","a134","a135","a136","a137","a138","a139","a140","a141","a142","a143","a144","a145","a146","a147","a148","a149","a150","a151","a152","a153","a154","a155","a156","a157","a158","a159","a160","a161","a162","a163","a164","a165","a166","a167","a168","a169","a170","a171","a172","a173","a174","a175","a176","a177","a178","a179","a180","a181","a182","a183","a184","a185","a186","a187","a188","a189","a190","a191","a192","a193","a194","a195","a196","a197","a198","a199","a200","a201","a202","a203","a204","a205","a206","a207","a208","a209","a210","a211","a212","a213","a214","a215","a216","a217","a218","a219","a220","a221","a222","a223","a224","a225","a226","a227","a228","a229","a230","a231","a232","a233","a234","a235","a236","a237","a238","a239","a240","a241","a242","a243","a244","a245","a246","a247","a248","a249","a250","a251","a252","a253","a254","a255"

typedef int v2i_t __attribute__((ext_vector_type(2)));

// The stage's scalar state lives in FIXED registers that the compiler never sees (an asm statement's scalar OUTPUT is a divergent value to hipcc
// and ends up in a VGPR): every group lists them as clobbers, and nothing but these strings reads or writes them.
//   s84 stages left in the DMA cursor's segment | s85 / s86 / s87 LDS slot of stage s / s + 1 / of the last finished stage | s88 / s89 this wave's
//   LDS-DMA destinations (G pieces, bit pieces) of stage s + QF_AHEAD | s90 / s91 byte offsets of that stage in G / in the block's columns of T |
//   s92 length of the DMA cursor's next segment | s93 bytes of T between stages | s94 / s95 end / start of the ring | s96 / s97 wave offsets of s88 / s89 |
//   s98 = 0x01010101, s99 = bytes of a slot (constants: an instruction with a 32-bit literal takes two issue slots)
#define QW_SREGS "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s93", "s94", "s95", "s96", "s97", "s98", "s99", "scc"

// the lane's own halves of the packed-bit words of one stage: H[tl][jp] = dwords of variant sub-tiles 2 jp, 2 jp + 1 of 64-sample tile tl
__device__ __forceinline__ void qw_read_bits(v2i_t (&H)[2][2], int h_addr)
{
    asm volatile("ds_read2st64_b32 %0, %4 offset1:1\n\tds_read2st64_b32 %1, %4 offset0:2 offset1:3\n\t"
                 "ds_read2st64_b32 %2, %4 offset0:16 offset1:17\n\tds_read2st64_b32 %3, %4 offset0:18 offset1:19"
                 : "+v"(H[0][0]), "+v"(H[0][1]), "+v"(H[1][0]), "+v"(H[1][1]) : "v"(h_addr) : "memory");
}

#include "lmm_quadform_wide_substeps.inc"

template <int ABL, int DM = 0, int PROF = 0>
__global__ __launch_bounds__(256, 1) void k_lmm_quadform_i8w(const int8_t *__restrict__ G, const uint64_t *__restrict__ T,
                                                              int64_t Vpad, int NR, int L, int lsplit, double *__restrict__ qout,
                                                              const int *__restrict__ nlimit, int nit_last, int nfull)
{
    constexpr int JT = 4, DMA_PER_WAVE = 6;
    extern __shared__ __attribute__((aligned(16))) char smem[];       // QF_NST slots x 24 KB
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    const int ntiles = (int)(Vpad / QF_BN);
    int tile, lgrp;
    if ((ntiles & 7) == 0) { const int xcd = blockIdx.x & 7, w = blockIdx.x >> 3; tile = (w / lsplit) * 8 + xcd; lgrp = w % lsplit; }
    else { tile = blockIdx.x / lsplit; lgrp = blockIdx.x % lsplit; }
    const int nl = (L - lgrp + lsplit - 1) / lsplit;
    const int64_t v0 = (int64_t)tile * QF_BN;
    if (nlimit && v0 >= (int64_t)*nlimit) return;
    asm volatile("" ::: QW_ALL_AGPRS);                                  // a[0:255] are this kernel's accumulators
    const int64_t TL = (int64_t)NR * (NR + 1);
    const uint32_t smem_base = (uint32_t)(uintptr_t)smem;              // LDS byte address of the ring
    const int aoff0 = qf_off(l31, lh), aoff1 = qf_off(l31, 2 + lh);     // row sub-tile it adds it * 2048 (the swizzle repeats every 32 rows)
    const int boff = 2 * QF_TILE_BYTES + (wave * (32 * JT) + l31) * 8;  // this lane's first variant column in the bits area (64-bit words)
    // LDS-DMA sources through two raw buffer descriptors (base G; base = the block's first column of T), so that a stage's source is ONE scalar
    // offset each (gso, tso) next to per-lane offsets that never change: 16 bytes per lane; G pieces 4 wave .. 4 wave + 3 (1 KB each), bit pieces
    // 2 wave, 2 wave + 1.  (The launcher keeps every offset below 2^32.)
    auto make_rsrc = [](const void *p) -> v4i {
        const uint64_t a = (uint64_t)(uintptr_t)p;
        return (v4i){__builtin_amdgcn_readfirstlane((int)(uint32_t)a), __builtin_amdgcn_readfirstlane((int)(uint32_t)((a >> 32) & 0xffffu)), -1, 0x00020000};
    };
    const v4i rsG = make_rsrc(G), rsT = make_rsrc(T + v0);
    uint32_t gvoff[4], tvoff[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) gvoff[j] = (uint32_t)((wave * 4 + j) * 1024 + lane * 16);
#pragma unroll
    for (int j = 0; j < 2; ++j) { const int pb = wave * 2 + j; tvoff[j] = (uint32_t)(((int64_t)(pb >> 2) * Vpad + (pb & 3) * 128 + lane * 2) * 8); }

    double tot[JT];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) tot[jt] = 0.0;
    double scale0 = 1.0;
    for (int i = 0; i < lgrp; ++i) scale0 *= 256.0;

    // DMA cursor (nl = 1: one limb per block, the launcher's condition for this kernel; the limb's stages are then contiguous in G): gso / tso = byte
    // offsets of the cursor's stage (two G tiles; the block's packed bits of the two 64-sample blocks they span).  The cursor runs QF_AHEAD stages
    // ahead and past the end of the stream by as much (into the next limb's tiles or the padding behind G; rows 0 .. 7 of T: NR >= 4 is the other
    // condition), so every stage issues the same six DMAs and the vmcnt arithmetic has no tail cases.
    // Where the launcher stops the stream short of NR segments (padding row tiles; a ragged one left to k_lmm_ragged_i8) the cursor runs on into the
    // next segment of the same limb: at least three segments run, so that one has four stages or more and spans rows 0 .. 7 of T at most.
    uint32_t gso = (uint32_t)((int64_t)lgrp * TL * QF_TILE_BYTES), tso = 0, prem = 1, plen = 2;
    const uint32_t tinc = (uint32_t)(2 * Vpad * 8);
    auto dma1 = [&](uint32_t lds_dst, uint32_t voff, const v4i &rs, uint32_t so) {
        if (!(ABL & 1)) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lds_dst), "v"(voff), "s"(rs), "s"(so) : "memory");
    };
    // prologue: stages 0 .. QF_AHEAD - 1 into slots 0 .. QF_AHEAD - 1
#pragma unroll 1
    for (int s = 0; s < QF_AHEAD; ++s) {
        const uint32_t dslot = smem_base + s * QF_STAGE_BYTES;
#pragma unroll
        for (int j = 0; j < 4; ++j) dma1(dslot + (wave * 4 + j) * 1024, gvoff[j], rsG, gso);
#pragma unroll
        for (int j = 0; j < 2; ++j) dma1(dslot + 2 * QF_TILE_BYTES + (wave * 2 + j) * 1024, tvoff[j], rsT, tso);
        gso += 2 * QF_TILE_BYTES; tso += tinc;
        if (--prem == 0) { tso = 0; prem = plen; ++plen; }
    }
    // stages 0 and 1 have landed for everybody
    if (!(ABL & 1)) qf_wait_vm<(QF_AHEAD - 2) * DMA_PER_WAVE>();
    __builtin_amdgcn_s_barrier();

    v4i AP[4], AQ[4], BP[4], BQ[4];
    v2i_t HC[2][2], HN[2][2];
#pragma unroll
    for (int it = 0; it < 4; ++it) { AP[it] = (v4i){0, 0, 0, 0}; AQ[it] = (v4i){0, 0, 0, 0}; }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { HC[a][b] = (v2i_t){0, 0}; HN[a][b] = (v2i_t){0, 0}; }
    {
        const int a0 = (int)smem_base + aoff0;
#pragma unroll
        for (int it = 0; it < 4; ++it) asm volatile("ds_read_b128 %0, %1 offset:%c2" : "+v"(AP[it]) : "v"(a0), "i"(it * 2048) : "memory");
        qw_read_bits(HC, (int)smem_base + boff + 4 * lh);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(AP[0]), "+v"(AP[1]), "+v"(AP[2]), "+v"(AP[3]), "+v"(HC[0][0]), "+v"(HC[0][1]), "+v"(HC[1][0]), "+v"(HC[1][1]));
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            const uint32_t h = (uint32_t)HC[0][jt >> 1][jt & 1];
            BP[jt] = (v4i){(int)(h & 0x01010101u), (int)((h >> 1) & 0x01010101u), (int)((h >> 2) & 0x01010101u), (int)((h >> 3) & 0x01010101u)};
        }
    }

    // The stream is walked as segments { first stage (C = 0) ; the other stages ; epilogue }: the common path holds no taken branch but the stage
    // loop's own.  A stage's values (ring slots, lane addresses, DMA destinations and source offsets) are prepared one stage ahead INSIDE the groups
    // of sub-steps 2 and 3 (QW_XS_*), three instructions at a time: a lone wavefront hides nothing anywhere else.
    const int boffl = boff + 4 * lh;
    int a0c = (int)smem_base + aoff0, a1c = (int)smem_base + aoff1;                                       // A fragment addresses in the current slot
    int a0n = a0c + QF_STAGE_BYTES, a1n = a1c + QF_STAGE_BYTES, hbn = (int)smem_base + QF_STAGE_BYTES + boffl;   // ... in the next one; this lane's bit words there
    asm volatile("s_mov_b32 s84, %0\n\ts_mov_b32 s85, %1\n\ts_add_u32 s86, %1, 0x6000\n\ts_mov_b32 s87, %1\n\t"
                 "s_add_u32 s88, %2, %3\n\ts_add_u32 s89, %2, %4\n\ts_mov_b32 s90, %5\n\ts_mov_b32 s91, %6\n\ts_mov_b32 s92, %7\n\ts_mov_b32 s93, %8\n\t"
                 "s_add_u32 s94, %1, %9\n\ts_mov_b32 s95, %1\n\ts_mov_b32 s96, %3\n\ts_mov_b32 s97, %4\n\ts_mov_b32 s98, 0x01010101\n\ts_mov_b32 s99, 0x6000"
                 ::"s"(prem), "s"(smem_base), "s"(smem_base + QF_AHEAD * QF_STAGE_BYTES), "s"(wave * 4096), "s"(2 * QF_TILE_BYTES + wave * 2048), "s"(gso),
                   "s"(tso), "s"(plen), "s"(tinc), "s"(QF_NST * QF_STAGE_BYTES) : QW_SREGS);
    uint64_t pt_wait = 0, pt_sub[4] = {0, 0, 0, 0}, pt_epi = 0, pt_tail = 0, pt0 = 0, pt1 = 0;   // PROF: s_memtime sums of wave 0
#define QW_STAMP(ACCU) if (PROF) { pt1 = __builtin_amdgcn_s_memtime(); ACCU += pt1 - pt0; pt0 = pt1; }
    if (PROF) pt0 = __builtin_amdgcn_s_memtime();

    // NIT = row sub-tiles (32 rows) the stage contracts: 4, or fewer in the LAST row tile when the sample count leaves most of it padding
    // (N = 5000: 8 valid rows of 128 -> one sub-tile, a quarter of the MFMAs in 40 of the 820 stages)
    auto stage = [&](auto zc, auto nc) {
        constexpr bool Z = decltype(zc)::value; constexpr int NIT = decltype(nc)::value;
#define QW_H(HH, TLX, JTX) ((uint32_t)HH[TLX][(JTX) >> 1][(JTX) & 1])
#define QW_BIND(AF, BF, RF, TLX, HH, ADDR, OFFV)                                                                                          \
        v4i(&A)[4] = AF; v4i(&B)[4] = BF; v4i(&R)[4] = RF; int N[4][4];                                                                    \
        const uint32_t H0 = QW_H(HH, TLX, 0), H1 = QW_H(HH, TLX, 1), H2 = QW_H(HH, TLX, 2), H3 = QW_H(HH, TLX, 3);                            \
        const int AA = ADDR; constexpr int OFF = OFFV;
#define QW_NEXT(BN) _Pragma("unroll") for (int it = 0; it < 4; ++it) BN[it] = (v4i){N[it][0], N[it][1], N[it][2], N[it][3]};
        const uint32_t(&GV)[4] = gvoff; const uint32_t(&TV)[2] = tvoff; const v4i &RSG = rsG, &RST = rsT;
        {   // ---- sub-step 0 (tile 0, k-half 0): A = AP, B = BP; next: (tile 0, k-half 1) -> AQ from a1c, BQ from HC[0] >> 4.
            // barrier_s sits behind the first MFMA: stages <= s + 1 have landed for every wave (two newer stages in flight) and nobody reads
            // stage s - 1 any more; its slot is refilled with stage s + QF_AHEAD by the DMAs that follow (four G pieces here, two bit pieces in 1)
            QW_BIND(AP, BP, AQ, 0, HC, a1c, 0)
            if (NIT == 4) {
                if (Z) { if (ABL & 1) QW_SUB0Z_NODMA(); else if (ABL & 16) QW_SUB0Z_NOBAR(); else QW_SUB0Z(); }
                else { if (ABL & 1) QW_SUB0_NODMA(); else if (ABL & 16) QW_SUB0_NOBAR(); else QW_SUB0(); }
            } else if (NIT == 2) {
                if (Z) { if (ABL & 1) QW_SUB0Z_NODMA_N2(); else if (ABL & 16) QW_SUB0Z_NOBAR_N2(); else QW_SUB0Z_N2(); }
                else { if (ABL & 1) QW_SUB0_NODMA_N2(); else if (ABL & 16) QW_SUB0_NOBAR_N2(); else QW_SUB0_N2(); }
            } else {
                if (Z) { if (ABL & 1) QW_SUB0Z_NODMA_N1(); else if (ABL & 16) QW_SUB0Z_NOBAR_N1(); else QW_SUB0Z_N1(); }
                else { if (ABL & 1) QW_SUB0_NODMA_N1(); else if (ABL & 16) QW_SUB0_NOBAR_N1(); else QW_SUB0_N1(); }
            }
            QW_NEXT(BQ)
        }
        QW_STAMP(pt_sub[0])
        {   // ---- sub-step 1 (tile 0, k-half 1): A = AQ, B = BQ; next: (tile 1, k-half 0) -> AP from a0c + 8192, BP from HC[1]
            QW_BIND(AQ, BQ, AP, 1, HC, a0c, 8192)
            if (NIT == 4) { if (ABL & 1) QW_SUB1_NODMA(); else QW_SUB1(); }
            else if (NIT == 2) { if (ABL & 1) QW_SUB1_NODMA_N2(); else QW_SUB1_N2(); }
            else { if (ABL & 1) QW_SUB1_NODMA_N1(); else QW_SUB1_N1(); }
            QW_NEXT(BP)
        }
        QW_STAMP(pt_sub[1])
        int a0n_n, a1n_n, hbn_n;
        {   // ---- sub-step 2 (tile 1, k-half 0): A = AP, B = BP; next: (tile 1, k-half 1) -> AQ from a1c + 8192, BQ from HC[1] >> 4.  The next
            // stage's bit words are requested early in it; the ring turns (next DMA destinations = the slot this stage reads)
            QW_BIND(AP, BP, AQ, 1, HC, a1c, 8192)
            const int HB = hbn, Y1 = aoff0; int X0;
            if (NIT == 4) QW_SUB2(); else if (NIT == 2) QW_SUB2_N2(); else QW_SUB2_N1();
            a0n_n = X0;
            QW_NEXT(BQ)
        }
        QW_STAMP(pt_sub[2])
        {   // ---- sub-step 3 (tile 1, k-half 1): A = AQ, B = BQ; next: stage s + 1 (tile 0, k-half 0) -> AP from the next slot, BP from HN[0];
            // the bit words of stage s + 1 become the current ones; the DMA cursor's source offsets move on
            QW_BIND(AQ, BQ, AP, 0, HN, a0n, 0)
            const int Y2 = aoff1, Y3 = boffl; int X1, X2;
            if (NIT == 4) QW_SUB3(); else if (NIT == 2) QW_SUB3_N2(); else QW_SUB3_N1();
            a1n_n = X1; hbn_n = X2;
            QW_NEXT(BP)
        }
#undef QW_H
        QW_STAMP(pt_sub[3])
        a0c = a0n; a1c = a1n; a0n = a0n_n; a1n = a1n_n; hbn = hbn_n;    // the names turn: what was "next" is "current" in the following stage
    };

    auto segment = [&](auto nc, int cI, double scale_l) {                    // one (row tile, limb): its stages, then the epilogue
        constexpr int NIT = decltype(nc)::value;
        if (ABL & 256) { if (cI == 0) stage(std::true_type{}, nc); else stage(std::false_type{}, nc); }     // timing ablation: never zeroed again
        else stage(std::true_type{}, nc);
#pragma unroll 1
        for (int k = 1; k <= cI; ++k) stage(std::false_type{}, nc);
        // ---- segment epilogue (see k_lmm_quadform_i8): sum_i x_i * acc_i over the 128 rows of tile cI, per variant column.  The full 64-bit
        // bit words of the segment's last stage (= the row tile's own samples) are read back from its slot, which nobody refills before the
        // next barrier.  One wavefront issues one instruction per ~4 cycles whatever it is, so the 3 x 256 instructions (accumulator read,
        // bit extract, 24-bit multiply-add) are ordered as four independent chains (the row sub-tiles) and no instruction waits for the one
        // in front of it.
            v4i W[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) W[a][b] = (v4i){0, 0, 0, 0};
        int wa;                                                         // the last finished stage's slot = the one in front of s85 in the ring
        asm volatile("s_cmp_eq_u32 s85, s95\n\ts_cselect_b32 s87, s94, s85\n\ts_sub_u32 s87, s87, s99\n\tv_add_u32 %0, s87, %1" : "=v"(wa) : "v"(boff) : QW_SREGS);
        asm volatile("ds_read2_b64 %[w0], %[p0] offset1:32\n\tds_read2_b64 %[w1], %[p0] offset0:64 offset1:96\n\t"
                     "ds_read2_b64 %[w2], %[p1] offset1:32\n\tds_read2_b64 %[w3], %[p1] offset0:64 offset1:96\n\t"
                     "s_waitcnt lgkmcnt(0)\n\ts_nop 7"
                     : [w0] "+v"(W[0][0]), [w1] "+v"(W[0][1]), [w2] "+v"(W[1][0]), [w3] "+v"(W[1][1]),
                       "+v"(AP[0]), "+v"(AP[1]), "+v"(AP[2]), "+v"(AP[3])
                     : [p0] "v"(wa), [p1] "v"(wa + QF_BN * 8) : "memory");
        if (ABL & 128) {
            int t0; asm volatile("v_accvgpr_read_b32 %0, a0" : "=v"(t0)); tot[0] += (double)(t0 + W[0][0][0]);
        } else {
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
                int part[4] = {0, 0, 0, 0};                     // (sub-tiles beyond NIT hold nothing of this segment)
                uint32_t w[4];
#pragma unroll
                for (int it = 0; it < 4; ++it)      // rows of row sub-tile it = samples 32 it .. of the stage: word (it >> 1), dword (it & 1) of sub-tile jt
                    w[it] = (uint32_t)W[it >> 1][jt >> 1][(jt & 1) * 2 + (it & 1)] >> (4 * lh);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2);
                    int t0, t1, t2, t3, b0, b1, b2, b3;             // |acc| <= 128 N / 2 < 2^23 (the launcher's conditions bound N far below 65536)
                    if (NIT == 4)
                        asm volatile("v_accvgpr_read_b32 %[t0], a%c[i0]\n\tv_accvgpr_read_b32 %[t1], a%c[i1]\n\t"
                                         "v_accvgpr_read_b32 %[t2], a%c[i2]\n\tv_accvgpr_read_b32 %[t3], a%c[i3]\n\t"
                                         "v_bfe_u32 %[b0], %[w0], %c[row], 1\n\tv_bfe_u32 %[b1], %[w1], %c[row], 1\n\t"
                                         "v_bfe_u32 %[b2], %[w2], %c[row], 1\n\tv_bfe_u32 %[b3], %[w3], %c[row], 1\n\t"
                                         "v_mad_i32_i24 %[p0], %[t0], %[b0], %[p0]\n\tv_mad_i32_i24 %[p1], %[t1], %[b1], %[p1]\n\t"
                                         "v_mad_i32_i24 %[p2], %[t2], %[b2], %[p2]\n\tv_mad_i32_i24 %[p3], %[t3], %[b3], %[p3]"
                                         : [p0] "+v"(part[0]), [p1] "+v"(part[1]), [p2] "+v"(part[2]), [p3] "+v"(part[3]), [t0] "=&v"(t0), [t1] "=&v"(t1),
                                           [t2] "=&v"(t2), [t3] "=&v"(t3), [b0] "=&v"(b0), [b1] "=&v"(b1), [b2] "=&v"(b2), [b3] "=&v"(b3)
                                         : [w0] "v"(w[0]), [w1] "v"(w[1]), [w2] "v"(w[2]), [w3] "v"(w[3]), [row] "i"(row), [i0] "i"((0 * 4 + jt) * 16 + r),
                                           [i1] "i"((1 * 4 + jt) * 16 + r), [i2] "i"((2 * 4 + jt) * 16 + r), [i3] "i"((3 * 4 + jt) * 16 + r));
                    else {
#pragma unroll
                        for (int it = 0; it < NIT; ++it) {
                            int t, bb;
                            if (it == 0) asm volatile("v_accvgpr_read_b32 %[t], a%c[i]\n\tv_bfe_u32 %[b], %[w], %c[row], 1\n\tv_mad_i32_i24 %[p], %[t], %[b], %[p]"
                                                      : [p] "+v"(part[0]), [t] "=&v"(t), [b] "=&v"(bb) : [w] "v"(w[0]), [row] "i"(row), [i] "i"((0 * 4 + jt) * 16 + r));
                            else asm volatile("v_accvgpr_read_b32 %[t], a%c[i]\n\tv_bfe_u32 %[b], %[w], %c[row], 1\n\tv_mad_i32_i24 %[p], %[t], %[b], %[p]"
                                              : [p] "+v"(part[1]), [t] "=&v"(t), [b] "=&v"(bb) : [w] "v"(w[1]), [row] "i"(row), [i] "i"((1 * 4 + jt) * 16 + r));
                        }
                    }
                }
                tot[jt] = fma((double)((part[0] + part[1]) + (part[2] + part[3])), scale_l, tot[jt]);
            }
        }
        QW_STAMP(pt_epi)
    };
    // nl = 1 (the launcher's condition): segment = row tile.  The launcher says how many of them run: `nfull` full ones (row tiles 0 .. nfull - 1) and,
    // behind them, one narrow one (nit_last = 2 or 1 row sub-tiles) or none (0): row tiles that are padding altogether are dropped, and so is a
    // ragged row tile that k_lmm_ragged_i8 contracts instead.  NR only describes the layout of G.
#pragma unroll 1
    for (int cI = 0; cI < nfull; ++cI) segment(std::integral_constant<int, 4>{}, cI, scale0);
    if (nit_last == 2) segment(std::integral_constant<int, 2>{}, nfull, scale0);
    else if (nit_last == 1) segment(std::integral_constant<int, 1>{}, nfull, scale0);
    const int nseg = nfull + (nit_last == 1 || nit_last == 2 ? 1 : 0), total = nl * (nseg * (nseg + 1) / 2);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");            // the re-fetched tail stages and the last prefetch
    if (PROF && blockIdx.x == 0 && tid == 0)
        printf("wide prof (block 0, wave 0): stages %d  wait %llu  sub0 %llu  sub1 %llu  sub2 %llu  sub3 %llu  tail %llu  epilogue %llu  (cycles)\n", total,
               (unsigned long long)pt_wait, (unsigned long long)pt_sub[0], (unsigned long long)pt_sub[1], (unsigned long long)pt_sub[2],
               (unsigned long long)pt_sub[3], (unsigned long long)pt_tail, (unsigned long long)pt_epi);
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) tot[jt] += __shfl_xor(tot[jt], 32, 64);
    if (lh == 0) {
        double *qo = qout + (int64_t)lgrp * Vpad + v0 + wave * (32 * JT) + l31;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) qo[32 * jt] = tot[jt];
    }
}
