// select_api.inc -- sh_select_* (include/seerhip.h): the rows of a packed cache restricted to, and permuted into, the samples of a run
// (included by api.hip inside its extern "C" block; the kernel: select_kernels.hip).
//
// A selector belongs to a context (its device, its N = n_dst) but owns a stream and its staging, like the device k-mer reader
// (kmer_api.inc): it runs on the reader's thread beside the context's job stream and lanes and never waits for them.
//   sh_select_rows        host rows in chunks of about 16 MB through two slots: chunk c is copied into pinned memory (the host pool; not for
//                         rows that lie in registered memory), goes up, through k_rows_select and back into pinned memory while chunk c - 1
//                         is copied out to the caller -- three PCIe crossings per row in all, counting the engine's own upload afterwards;
//   sh_select_rows_dev    rows that are on the device already: one launch on the selector's stream, complete when the call returns;
//   sh_select_rows_host   the same rule in plain C++ on the host pool, no context: the CPU tests, and the rate to compare against.
hipError_t shk_rows_select(hipStream_t, const void *, int64_t, int64_t, const int32_t *, int, void *, int32_t *);
int64_t shk_rows_select_max_row_bytes(void);
//   sh_select_calls / _dev / _host   the same three for a block of CALLS (a call cache, DESIGN.md section 5.9): a present and a missing plane of the
//                         same rows through k_calls_select, which shares one load of the map between both; the two planes of a chunk lie behind
//                         one another in a slot's buffers, [present rows | missing rows], and so do their counts.
//   sh_job_submit_calls_select (job_api.inc) takes the selector's staging and stream for a block on its way into a job's slot.
hipError_t shk_calls_select(hipStream_t, const void *, const void *, int64_t, int64_t, const int32_t *, int, void *, void *, int32_t *, int32_t *);
int64_t shk_calls_select_max_row_bytes(void);

#define SELECT_CHUNK_BYTES ((int64_t)16 << 20)

struct sh_select {
    sh_ctx *ctx = nullptr; int device = 0, n_src = 0, n_dst = 0;
    hipStream_t stream = nullptr;
    uint64_t job_blocks = 0;                               // blocks sh_job_submit_calls_select has staged: block b through slot[b & 1]
    hipEvent_t t0 = nullptr, t1 = nullptr; bool timed = false;   // around the last launch of sh_select_calls_dev (sh_select_kernel_ms)
    int32_t *d_map = nullptr;
    struct Slot { uint8_t *h_in = nullptr, *d_in = nullptr, *h_out = nullptr, *d_out = nullptr; int32_t *h_counts = nullptr, *d_counts = nullptr;
                  int64_t cap_in = 0, cap_rows = 0, cap_rows_dev = 0; hipEvent_t done = nullptr, used = nullptr; } slot[2];
};

// every entry in [0, n_src), no entry twice
static int select_check_map(int n_src, const int32_t *map, int n_dst, const char *who)
{
    if (n_src < 1 || n_dst < 1 || !map) return fail(SH_EINVAL, std::string(who) + ": bad argument");
    if (n_dst > n_src) return fail(SH_ESHAPE, std::string(who) + ": more samples selected than the rows hold");
    std::vector<uint8_t> seen((size_t)n_src, 0);
    for (int j = 0; j < n_dst; ++j) {
        if (map[j] < 0 || map[j] >= n_src) return fail(SH_EINVAL, std::string(who) + ": map entry " + std::to_string(j) + " is outside the source row (" + std::to_string(map[j]) + ")");
        if (seen[(size_t)map[j]]) return fail(SH_EINVAL, std::string(who) + ": source sample " + std::to_string(map[j]) + " is selected twice");
        seen[(size_t)map[j]] = 1;
    }
    return SH_OK;
}

static int select_check_rows(int n_src, int64_t src_row_bytes, int64_t V, const void *in, const void *out, const void *counts, const char *who)
{
    if (V < 0 || src_row_bytes <= 0 || (V > 0 && (!in || !out || !counts))) return fail(SH_EINVAL, std::string(who) + ": bad argument");
    if (src_row_bytes & 7) return fail(SH_ESHAPE, std::string(who) + ": src_row_bytes must be a multiple of 8");
    if (src_row_bytes * 8 < n_src) return fail(SH_ESHAPE, std::string(who) + ": src_row_bytes*8 < n_src");
    return SH_OK;
}

void sh_select_close(sh_select *s)
{
    if (!s) return;
    hipSetDevice(s->device);
    if (s->stream) hipStreamSynchronize(s->stream);
    for (auto &sl : s->slot) {
        if (sl.h_in) hipHostFree(sl.h_in);
        if (sl.h_out) hipHostFree(sl.h_out);
        if (sl.h_counts) hipHostFree(sl.h_counts);
        hipFree(sl.d_in); hipFree(sl.d_out); hipFree(sl.d_counts);
        if (sl.done) hipEventDestroy(sl.done);
        if (sl.used) hipEventDestroy(sl.used);
    }
    hipFree(s->d_map);
    if (s->t0) hipEventDestroy(s->t0);
    if (s->t1) hipEventDestroy(s->t1);
    if (s->stream) hipStreamDestroy(s->stream);
    delete s;
}

static int select_open_device(sh_select *s, const int32_t *map)
{
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    for (auto &sl : s->slot) { HIPCHK(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&sl.used, hipEventDisableTiming)); }
    HIPCHK(dmalloc(&s->d_map, (size_t)s->n_dst));
    HIPCHK(hipMemcpyAsync(s->d_map, map, (size_t)s->n_dst * 4, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));                // (the caller's table is pageable and its own again from here on)
    return SH_OK;
}

sh_select *sh_select_open(sh_ctx *ctx, int n_src, const int32_t *map, int n_dst)
{
    if (!ctx) { fail(SH_EINVAL, "sh_select_open: null ctx"); return nullptr; }
    if (ctx->N != n_dst) { fail(SH_ESHAPE, "sh_select_open: the context was created for another number of samples than the map selects"); return nullptr; }
    if (select_check_map(n_src, map, n_dst, "sh_select_open") != SH_OK) return nullptr;
    if ((((int64_t)n_src + 63) / 64) * 8 > shk_rows_select_max_row_bytes()) {
        fail(SH_ESHAPE, "sh_select_open: too many source samples for k_rows_select's row in LDS (at most " + std::to_string(shk_rows_select_max_row_bytes() * 8) + ")");
        return nullptr;
    }
    sh_select *s = new sh_select();
    s->ctx = ctx; s->device = ctx->device; s->n_src = n_src; s->n_dst = n_dst;
    if (select_open_device(s, map) != SH_OK) { const std::string keep = g_err; sh_select_close(s); fail(SH_EHIP, keep); return nullptr; }
    return s;
}

// stage_out: the rows and counts come back to the host (pinned h_out, h_counts); without it the slot's outputs stay on the device
static int select_ensure(sh_select *s, sh_select::Slot &sl, int64_t rows, int64_t in_bytes, bool stage_in, bool stage_out = true)
{
    const int64_t out_rb = (((int64_t)s->n_dst + 63) / 64) * 8;
    if (in_bytes > sl.cap_in) {
        HIPCHK(hipStreamSynchronize(s->stream));
        if (sl.h_in) hipHostFree(sl.h_in);
        hipFree(sl.d_in); sl.h_in = sl.d_in = nullptr; sl.cap_in = 0;
        HIPCHK(hipMalloc((void **)&sl.d_in, (size_t)in_bytes));
        sl.cap_in = in_bytes;
    }
    if (stage_in && !sl.h_in) HIPCHK(hipHostMalloc((void **)&sl.h_in, (size_t)sl.cap_in, hipHostMallocDefault));
    if (stage_out && rows > sl.cap_rows) {
        HIPCHK(hipStreamSynchronize(s->stream));
        if (sl.h_out) hipHostFree(sl.h_out);
        if (sl.h_counts) hipHostFree(sl.h_counts);
        sl.h_out = nullptr; sl.h_counts = nullptr; sl.cap_rows = 0;
        HIPCHK(hipHostMalloc((void **)&sl.h_out, (size_t)(rows * out_rb), hipHostMallocDefault));
        HIPCHK(hipHostMalloc((void **)&sl.h_counts, (size_t)rows * 4, hipHostMallocDefault));
        sl.cap_rows = rows;
    }
    if (rows > sl.cap_rows_dev) {
        HIPCHK(hipStreamSynchronize(s->stream));
        hipFree(sl.d_out); hipFree(sl.d_counts);
        sl.d_out = nullptr; sl.d_counts = nullptr; sl.cap_rows_dev = 0;
        HIPCHK(hipMalloc((void **)&sl.d_out, (size_t)(rows * out_rb)));
        HIPCHK(dmalloc(&sl.d_counts, (size_t)rows));
        sl.cap_rows_dev = rows;
    }
    return SH_OK;
}

// nbytes from src to dst on the host pool, in pieces of 1 MB
static void select_copy(uint8_t *dst, const uint8_t *src, int64_t nbytes)
{
    const int64_t piece = (int64_t)1 << 20, n = (nbytes + piece - 1) / piece;
    const std::function<void(int64_t)> fn = [&](int64_t i) { memcpy(dst + i * piece, src + i * piece, (size_t)std::min(piece, nbytes - i * piece)); };
    shost::CpuScope cs(shost::ST_STAGE_COPY);
    shost::pool().run(n, 1, fn, shost::ST_STAGE_COPY, shost::per_stream_cpus());
}

int sh_select_rows(sh_select *s, const uint8_t *bits, int64_t src_row_bytes, int64_t V, uint8_t *out_bits, int32_t *out_counts, int src_is_dma)
{
    if (!s) return fail(SH_EINVAL, "sh_select_rows: null selector");
    const int rc0 = select_check_rows(s->n_src, src_row_bytes, V, bits, out_bits, out_counts, "sh_select_rows"); if (rc0) return rc0;
    if (src_row_bytes > shk_rows_select_max_row_bytes()) return fail(SH_ESHAPE, "sh_select_rows: the source row is too wide for k_rows_select's row in LDS");
    if (V == 0) return SH_OK;
    HIPCHK(hipSetDevice(s->device));
    const int64_t out_rb = (((int64_t)s->n_dst + 63) / 64) * 8;
    const int64_t chunk = std::max<int64_t>(1, SELECT_CHUNK_BYTES / src_row_bytes), n_chunks = (V + chunk - 1) / chunk;
    // chunk c's results are complete (its slot's event) and go to the caller
    auto finish = [&](int64_t c) -> int {
        sh_select::Slot &sl = s->slot[c & 1];
        const int64_t v0 = c * chunk, nv = std::min(chunk, V - v0);
        HIPCHK(hipEventSynchronize(sl.done));
        select_copy(out_bits + v0 * out_rb, sl.h_out, nv * out_rb);
        memcpy(out_counts + v0, sl.h_counts, (size_t)nv * 4);
        return SH_OK;
    };
    for (int64_t c = 0; c < n_chunks; ++c) {
        sh_select::Slot &sl = s->slot[c & 1];
        if (c >= 2) { const int rc = finish(c - 2); if (rc) return rc; }
        const int64_t v0 = c * chunk, nv = std::min(chunk, V - v0);
        const int rc = select_ensure(s, sl, std::min(chunk, V), std::min(chunk, V) * src_row_bytes, !src_is_dma); if (rc) return rc;
        const uint8_t *from = bits + v0 * src_row_bytes;
        if (!src_is_dma) { select_copy(sl.h_in, from, nv * src_row_bytes); from = sl.h_in; }
        HIPCHK(hipMemcpyAsync(sl.d_in, from, (size_t)(nv * src_row_bytes), hipMemcpyHostToDevice, s->stream));
        HIPCHK(shk_rows_select(s->stream, sl.d_in, src_row_bytes, nv, s->d_map, s->n_dst, sl.d_out, sl.d_counts));
        HIPCHK(hipMemcpyAsync(sl.h_out, sl.d_out, (size_t)(nv * out_rb), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipMemcpyAsync(sl.h_counts, sl.d_counts, (size_t)nv * 4, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipEventRecord(sl.done, s->stream));
    }
    for (int64_t c = std::max<int64_t>(0, n_chunks - 2); c < n_chunks; ++c) { const int rc = finish(c); if (rc) return rc; }
    return SH_OK;
}

int sh_select_rows_dev(sh_select *s, const void *d_bits, int64_t src_row_bytes, int64_t V, void *d_out, int32_t *d_counts)
{
    if (!s) return fail(SH_EINVAL, "sh_select_rows_dev: null selector");
    const int rc0 = select_check_rows(s->n_src, src_row_bytes, V, d_bits, d_out, d_counts, "sh_select_rows_dev"); if (rc0) return rc0;
    if (src_row_bytes > shk_rows_select_max_row_bytes()) return fail(SH_ESHAPE, "sh_select_rows_dev: the source row is too wide for k_rows_select's row in LDS");
    if ((((uintptr_t)d_bits) | ((uintptr_t)d_out)) & 7) return fail(SH_EINVAL, "sh_select_rows_dev: rows must be 8-byte aligned");
    if (V == 0) return SH_OK;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(shk_rows_select(s->stream, d_bits, src_row_bytes, V, s->d_map, s->n_dst, d_out, d_counts));
    HIPCHK(hipStreamSynchronize(s->stream));
    return SH_OK;
}

// Host rows of the cache's width into the context's similarity accumulator: every row goes up once and nothing comes back.  Chunks of about
// 128 MB alternate between the two slots: chunk c is copied into the slot's pinned memory, uploaded and selected on the selector's stream
// (event `done`); the context's stream waits for that event, accumulates the selected rows (sh_sim_accumulate_dev) and records `used`, which
// the selector's stream waits for before it writes the slot's rows again -- so chunk c + 1 is staged, uploaded and selected under chunk c's
// accumulation.  The chunks are large because every accumulation adds whole tiles of K (sim_kernels.hip k_sim_pairs).
#define SIM_SELECT_CHUNK_BYTES ((int64_t)128 << 20)

int sh_sim_accumulate_select(sh_ctx *c, sh_select *s, const uint8_t *bits, int64_t src_row_bytes, int64_t V)
{
    if (!s) return fail(SH_EINVAL, "sh_sim_accumulate_select: null selector");
    if (!c || c != s->ctx) return fail(SH_EINVAL, "sh_sim_accumulate_select: the selector belongs to another context");
    if (!c->sim_K) return fail(SH_EINVAL, "sh_sim_begin has not run");
    const int rc0 = select_check_rows(s->n_src, src_row_bytes, V, bits, bits, bits, "sh_sim_accumulate_select"); if (rc0) return rc0;
    if (src_row_bytes > shk_rows_select_max_row_bytes()) return fail(SH_ESHAPE, "sh_sim_accumulate_select: the source row is too wide for k_rows_select's row in LDS");
    if (V == 0) return SH_OK;
    HIPCHK(hipSetDevice(s->device));
    const int64_t out_rb = (((int64_t)s->n_dst + 63) / 64) * 8;
    const int64_t chunk = std::max<int64_t>(1, SIM_SELECT_CHUNK_BYTES / src_row_bytes), n_chunks = (V + chunk - 1) / chunk;
    for (int64_t ci = 0; ci < n_chunks; ++ci) {
        sh_select::Slot &sl = s->slot[ci & 1];
        const int64_t v0 = ci * chunk, nv = std::min(chunk, V - v0);
        if (ci >= 2) HIPCHK(hipEventSynchronize(sl.done));                 // (the slot's pinned rows have gone up)
        int rc = select_ensure(s, sl, std::min(chunk, V), std::min(chunk, V) * src_row_bytes, true, false); if (rc) return rc;
        select_copy(sl.h_in, bits + v0 * src_row_bytes, nv * src_row_bytes);
        if (ci >= 2) HIPCHK(hipStreamWaitEvent(s->stream, sl.used, 0));    // (the slot's selected rows have been accumulated)
        HIPCHK(hipMemcpyAsync(sl.d_in, sl.h_in, (size_t)(nv * src_row_bytes), hipMemcpyHostToDevice, s->stream));
        HIPCHK(shk_rows_select(s->stream, sl.d_in, src_row_bytes, nv, s->d_map, s->n_dst, sl.d_out, sl.d_counts));
        HIPCHK(hipEventRecord(sl.done, s->stream));
        HIPCHK(hipStreamWaitEvent(c->stream, sl.done, 0));
        rc = sh_sim_accumulate_dev(c, sl.d_out, out_rb, nv); if (rc) return rc;
        HIPCHK(hipEventRecord(sl.used, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));                               // (which has waited for every chunk's selection)
    return SH_OK;
}

// the kernel's rule in plain C++: out bit j = source bit map[j]; whole output rows are written, pad bits zero
static int select_rows_host(const uint8_t *bits, int64_t src_row_bytes, int64_t V, int n_src, const int32_t *map, int n_dst, uint8_t *out_bits, int32_t *out_counts,
                            const char *who)
{
    const int rc0 = select_check_map(n_src, map, n_dst, who); if (rc0) return rc0;
    if (V < 0 || src_row_bytes <= 0 || (V > 0 && (!bits || !out_bits || !out_counts))) return fail(SH_EINVAL, std::string(who) + ": bad argument");
    if (src_row_bytes * 8 < n_src) return fail(SH_ESHAPE, std::string(who) + ": src_row_bytes*8 < n_src");
    const int64_t out_rb = (((int64_t)n_dst + 63) / 64) * 8;
    const int out_words = (n_dst + 63) >> 6;
    const std::function<void(int64_t)> fn = [&](int64_t v) {
        const uint8_t *row = bits + v * src_row_bytes;
        uint8_t *o = out_bits + v * out_rb;
        int cnt = 0;
        for (int w = 0; w < out_words; ++w) {
            uint64_t word = 0;
            const int n = std::min(64, n_dst - 64 * w);
            const int32_t *m = map + 64 * w;
            for (int l = 0; l < n; ++l) word |= (uint64_t)((row[m[l] >> 3] >> (m[l] & 7)) & 1u) << l;
            cnt += __builtin_popcountll(word);
            memcpy(o + 8 * w, &word, 8);
        }
        out_counts[v] = cnt;
    };
    shost::CpuScope cs(shost::ST_OTHER);
    shost::pool().run(V, 64, fn, shost::ST_OTHER);
    return SH_OK;
}

int sh_select_rows_host(const uint8_t *bits, int64_t src_row_bytes, int64_t V, int n_src, const int32_t *map, int n_dst, uint8_t *out_bits, int32_t *out_counts)
{
    return select_rows_host(bits, src_row_bytes, V, n_src, map, n_dst, out_bits, out_counts, "sh_select_rows_host");
}

// ---- blocks of calls: two planes of the same rows (k_calls_select) ---------------------------------------------------------------------------
static int select_check_calls(sh_select *s, int64_t src_row_bytes, int64_t V, const void *p, const void *m, const void *op, const void *om, const void *np,
                              const void *nm, const char *who)
{
    if (!s) return fail(SH_EINVAL, std::string(who) + ": null selector");
    int rc = select_check_rows(s->n_src, src_row_bytes, V, p, op, np, who); if (rc) return rc;
    rc = select_check_rows(s->n_src, src_row_bytes, V, m, om, nm, who); if (rc) return rc;
    if (src_row_bytes > shk_calls_select_max_row_bytes())
        return fail(SH_ESHAPE, std::string(who) + ": the source row is too wide for the two planes of one wavefront of k_calls_select in LDS (at most " +
                               std::to_string(shk_calls_select_max_row_bytes()) + " bytes)");
    return SH_OK;
}

int sh_select_calls(sh_select *s, const uint8_t *present, const uint8_t *missing, int64_t src_row_bytes, int64_t V, uint8_t *out_present, uint8_t *out_missing,
                    int32_t *out_n_present, int32_t *out_n_missing)
{
    const int rc0 = select_check_calls(s, src_row_bytes, V, present, missing, out_present, out_missing, out_n_present, out_n_missing, "sh_select_calls"); if (rc0) return rc0;
    if (V == 0) return SH_OK;
    HIPCHK(hipSetDevice(s->device));
    const int64_t out_rb = (((int64_t)s->n_dst + 63) / 64) * 8;
    const int64_t chunk = std::max<int64_t>(1, SELECT_CHUNK_BYTES / (2 * src_row_bytes)), n_chunks = (V + chunk - 1) / chunk, cap = std::min(chunk, V);
    auto finish = [&](int64_t c) -> int {
        sh_select::Slot &sl = s->slot[c & 1];
        const int64_t v0 = c * chunk, nv = std::min(chunk, V - v0);
        HIPCHK(hipEventSynchronize(sl.done));
        select_copy(out_present + v0 * out_rb, sl.h_out, nv * out_rb);
        select_copy(out_missing + v0 * out_rb, sl.h_out + cap * out_rb, nv * out_rb);
        memcpy(out_n_present + v0, sl.h_counts, (size_t)nv * 4);
        memcpy(out_n_missing + v0, sl.h_counts + cap, (size_t)nv * 4);
        return SH_OK;
    };
    for (int64_t c = 0; c < n_chunks; ++c) {
        sh_select::Slot &sl = s->slot[c & 1];
        if (c >= 2) { const int rc = finish(c - 2); if (rc) return rc; }
        const int64_t v0 = c * chunk, nv = std::min(chunk, V - v0);
        // (a slot holds `cap` rows of each plane: the missing plane, its output and its counts start `cap` rows in)
        const int rc = select_ensure(s, sl, 2 * cap, 2 * cap * src_row_bytes, true); if (rc) return rc;
        select_copy(sl.h_in, present + v0 * src_row_bytes, nv * src_row_bytes);
        select_copy(sl.h_in + cap * src_row_bytes, missing + v0 * src_row_bytes, nv * src_row_bytes);
        HIPCHK(hipMemcpyAsync(sl.d_in, sl.h_in, (size_t)(nv * src_row_bytes), hipMemcpyHostToDevice, s->stream));
        HIPCHK(hipMemcpyAsync(sl.d_in + cap * src_row_bytes, sl.h_in + cap * src_row_bytes, (size_t)(nv * src_row_bytes), hipMemcpyHostToDevice, s->stream));
        HIPCHK(shk_calls_select(s->stream, sl.d_in, sl.d_in + cap * src_row_bytes, src_row_bytes, nv, s->d_map, s->n_dst, sl.d_out, sl.d_out + cap * out_rb,
                                sl.d_counts, sl.d_counts + cap));
        HIPCHK(hipMemcpyAsync(sl.h_out, sl.d_out, (size_t)((cap + nv) * out_rb), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipMemcpyAsync(sl.h_counts, sl.d_counts, (size_t)(cap + nv) * 4, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipEventRecord(sl.done, s->stream));
    }
    for (int64_t c = std::max<int64_t>(0, n_chunks - 2); c < n_chunks; ++c) { const int rc = finish(c); if (rc) return rc; }
    return SH_OK;
}

int sh_select_calls_dev(sh_select *s, const void *d_present, const void *d_missing, int64_t src_row_bytes, int64_t V, void *d_out_present, void *d_out_missing,
                        int32_t *d_n_present, int32_t *d_n_missing)
{
    const int rc0 = select_check_calls(s, src_row_bytes, V, d_present, d_missing, d_out_present, d_out_missing, d_n_present, d_n_missing, "sh_select_calls_dev");
    if (rc0) return rc0;
    if ((((uintptr_t)d_present) | ((uintptr_t)d_missing) | ((uintptr_t)d_out_present) | ((uintptr_t)d_out_missing)) & 7)
        return fail(SH_EINVAL, "sh_select_calls_dev: rows must be 8-byte aligned");
    if (V == 0) return SH_OK;
    HIPCHK(hipSetDevice(s->device));
    if (!s->t0) { HIPCHK(hipEventCreate(&s->t0)); HIPCHK(hipEventCreate(&s->t1)); }
    HIPCHK(hipEventRecord(s->t0, s->stream));
    HIPCHK(shk_calls_select(s->stream, d_present, d_missing, src_row_bytes, V, s->d_map, s->n_dst, d_out_present, d_out_missing, d_n_present, d_n_missing));
    HIPCHK(hipEventRecord(s->t1, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->timed = true;
    return SH_OK;
}

// milliseconds between the stream events around the launch of the last sh_select_calls_dev (the measurement: tools/calls_cache_bench.py)
int sh_select_kernel_ms(sh_select *s, double *ms)
{
    if (!s || !ms) return fail(SH_EINVAL, "sh_select_kernel_ms: null argument");
    if (!s->timed) return fail(SH_EINVAL, "sh_select_kernel_ms: sh_select_calls_dev has not run");
    float t = 0.0f;
    HIPCHK(hipEventElapsedTime(&t, s->t0, s->t1));
    *ms = (double)t;
    return SH_OK;
}

int sh_select_calls_host(const uint8_t *present, const uint8_t *missing, int64_t src_row_bytes, int64_t V, int n_src, const int32_t *map, int n_dst,
                         uint8_t *out_present, uint8_t *out_missing, int32_t *out_n_present, int32_t *out_n_missing)
{
    const int rc = select_rows_host(present, src_row_bytes, V, n_src, map, n_dst, out_present, out_n_present, "sh_select_calls_host"); if (rc) return rc;
    return select_rows_host(missing, src_row_bytes, V, n_src, map, n_dst, out_missing, out_n_missing, "sh_select_calls_host");
}

// A stored block of a call cache over n_src samples into the job stream of a run over n_dst of them (sh_job_submit_calls with the selection in
// front).  The source planes go into the selector's pinned slot b & 1 and up, once, on the selector's stream; k_calls_select writes the selected
// planes and their counts straight into the job slot's device buffer, in calls_layout; `skip` goes up beside them through the job slot's pinned
// slab, and the counts -- with the planes only when the job lists samples (sh_job_set_samples reads them on the host) -- come back into that
// slab.  The slot's ev_h2d is recorded on the selector's stream behind all of it, and the stream that runs the block's kernels waits for it,
// as it waits for a plain block's upload.  The job slot's device buffer is free when this is called: its last block was collected, behind
// its ev_done.  A selector slot's pinned rows are written again once the event behind their last upload and kernel has passed.
int sh_job_submit_calls_select(sh_job *j, sh_select *sel, const uint8_t *present, const uint8_t *missing, int64_t src_row_bytes, int64_t V, const int32_t *skip,
                               const char *names, const int64_t *name_off, double max_missing)
{
    if (!j) return fail(SH_EINVAL, "null job");
    if (!sel) return fail(SH_EINVAL, "sh_job_submit_calls_select: null selector");
    if (sel->ctx != j->c) return fail(SH_EINVAL, "sh_job_submit_calls_select: the selector belongs to another context");
    if (!present || !missing || !skip || !names || !name_off || V <= 0) return fail(SH_EINVAL, "sh_job_submit_calls_select: bad argument");
    int rc = select_check_calls(sel, src_row_bytes, V, present, missing, present, missing, skip, skip, "sh_job_submit_calls_select"); if (rc) return rc;
    if (j->n_submitted - j->n_collected >= (uint64_t)j->depth) return fail(SH_EINVAL, "sh_job_submit_calls_select: every slot holds a block; collect one first");
    sh_ctx *c = j->c;
    HIPCHK(hipSetDevice(c->device));
    const int64_t out_rb = (((int64_t)sel->n_dst + 63) / 64) * 8;
    JobSlot &s = j->slot[j->n_submitted % j->depth];
    rc = job_ensure(j, s, V, out_rb, true, true); if (rc) return rc;
    sh_select::Slot &sl = sel->slot[sel->job_blocks & 1];
    if (sel->job_blocks >= 2) { rc = wait_event_asleep(sl.done); if (rc) return rc; }   // (the slot's pinned rows have gone up; hipEventSynchronize spins a CPU)
    rc = select_ensure(sel, sl, 0, 2 * V * src_row_bytes, true, false); if (rc) return rc;
    const CallsLayout CL = calls_layout(V, out_rb);
    const bool lists = !j->smp_order.empty();
    s.bits = s.hp_bits; s.miss = s.hp_bits + CL.miss; s.row_bytes = out_rb; s.V = V; s.names = names; s.name_off = name_off;
    s.calls = 1; s.counts_from_device = 1; s.max_missing = max_missing; s.no_last_lineage = skip[V - 1] != 0 ? 1 : 0;
    s.cnt_host.assign((size_t)V, 0);
    s.counts = s.cnt_host.data();
    int32_t *h_ints = (int32_t *)(s.hp_bits + CL.ints);
    select_copy(sl.h_in, present, V * src_row_bytes);
    select_copy(sl.h_in + V * src_row_bytes, missing, V * src_row_bytes);
    std::memcpy(h_ints + 2 * V, skip, (size_t)V * 4);
    {
        shost::CpuScope cs(shost::ST_SUBMIT);
        int32_t *d_ints = (int32_t *)(s.d_bits + CL.ints);
        HIPCHK(hipMemcpyAsync(sl.d_in, sl.h_in, (size_t)(2 * V * src_row_bytes), hipMemcpyHostToDevice, sel->stream));
        HIPCHK(hipMemcpyAsync(d_ints + 2 * V, h_ints + 2 * V, (size_t)V * 4, hipMemcpyHostToDevice, sel->stream));
        if (CL.ints > 2 * CL.miss) { HIPCHK(hipMemsetAsync(s.d_bits + 2 * CL.miss, 0, CL.ints - 2 * CL.miss, sel->stream)); }   // (the pad: zeros, as sh_job_submit_calls uploads them)
        HIPCHK(shk_calls_select(sel->stream, sl.d_in, sl.d_in + V * src_row_bytes, src_row_bytes, V, sel->d_map, sel->n_dst, s.d_bits, s.d_bits + CL.miss, d_ints, d_ints + V));
        HIPCHK(hipEventRecord(sl.done, sel->stream));
        HIPCHK(hipMemcpyAsync(h_ints, d_ints, (size_t)V * 8, hipMemcpyDeviceToHost, sel->stream));
        if (lists) { HIPCHK(hipMemcpyAsync(s.hp_bits, s.d_bits, 2 * CL.miss, hipMemcpyDeviceToHost, sel->stream)); }
        HIPCHK(hipEventRecord(s.ev_h2d, sel->stream));
    }
    ++sel->job_blocks;
    s.state = 1;
    ++j->n_submitted;
    while (j->n_computed + (j->lanes > 1 ? 0 : 1) < j->n_submitted) {    // (as sh_job_submit hands the blocks' kernels over)
        rc = job_compute(j, j->slot[j->n_computed % j->depth]); if (rc) return rc;
        ++j->n_computed;
    }
    return SH_OK;
}
