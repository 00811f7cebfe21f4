// job_api.inc -- the job stream (round 5; included by api.hip inside its extern "C" block): blocks of packed rows in, the TSV text of the
// rows the run prints + the run's counters out, pipelined three deep, with the host touching only PRINTED rows.
//
// What it replaces: the per-block Python of pyseer_amd/__main__.py run_stream (engine call with host result arrays -> mask_like_fit_lmm ->
// numpy selects and counters over every tested row -> sh_format_rows), i.e. the reference's print loops pyseer/__main__.py:571-593, 805-827
// and format_output (pyseer/utils.py:39-105).  Per block, host side: one hipMemcpyAsync of the rows (DMA straight out of the caller's
// registered memory -- sh_host_register on the packed-cache mapping -- or through a pinned slab filled by the process-wide pool), the batch's
// kernel launches, one wait with the thread asleep (wait_event_asleep: hipStreamSynchronize / hipEventSynchronize spin a whole CPU per waiting
// stream), and the
// formatting of the selected records.  Ring of SH_JOB_DEPTH slots: the rows of block k cross PCIe while block k-1 runs its kernels and block
// k-2 is formatted and written by the caller.  A fixed-effects job computes its blocks on the context's LANES (lanes_api.inc: the launch
// code of a fixed-effects batch blocks on list-length read-backs, and one stream leaves the device idle between its small kernels), so its
// ring is n_lanes slots deeper and the kernels of consecutive blocks run side by side.
#define SH_JOB_DEPTH 3
#define SH_JOB_MAX_DEPTH (SH_JOB_DEPTH + 8)

struct JobSlot {
    uint8_t *d_bits = nullptr; int64_t cap_bits = 0;
    double *d_out = nullptr; uint32_t *d_flags = nullptr; int *d_bcount = nullptr; long long *d_hdr = nullptr; int64_t cap_rows = 0; int cap_nrow = 0;
    uint8_t *hp_bits = nullptr; int64_t cap_hp = 0;                    // pinned slab for rows that are not DMA-able where they lie
    uint8_t *h_res = nullptr; int64_t cap_res_rows = 0; int res_nrow = 0;   // host-mapped: header, idx, flags, cols, lineage (the scatter kernel's target)
    int32_t *d_sel = nullptr; int64_t cap_sel = 0;                      // lineage: the printed rows' indices, on the device
    uint64_t *d_T1 = nullptr;                                           // lineage of the block's LAST row (LMM, lmm.py:209-213): that row repacked alone
    uint32_t *d_dig = nullptr; char *d_pat = nullptr; char *h_pat = nullptr; int64_t cap_pat = 0;   // --output-patterns: digests, their text on the device and pinned
    hipEvent_t ev_h2d = nullptr, ev_done = nullptr;
    // the block in the slot
    const uint8_t *bits = nullptr; int64_t row_bytes = 0, V = 0; const int32_t *counts = nullptr; const char *names = nullptr; const int64_t *name_off = nullptr;
    int state = 0;                                                      // 0 free, 1 rows on their way, 2 kernels queued, 3 the lane that ran them failed
    int rc = 0; std::string err;                                        // (state 3)
};

struct sh_job {
    sh_ctx *c = nullptr; int lmm = 0, print_filtered = 0, q = 0, nrow = 5;
    JobSlot slot[SH_JOB_MAX_DEPTH];
    int depth = SH_JOB_DEPTH, lanes = 1;
    std::mutex mu; std::condition_variable cv;                          // slot states written by lane threads
    uint64_t n_submitted = 0, n_computed = 0, n_collected = 0;
    hipStream_t copy_stream = nullptr;
    std::vector<uint8_t> valid;                                         // per printed row: are the covariate slopes printed
    // fit_lineage_effect inside the stream (sh_job_set_lineage): 0 off; 1 every printed row the reference fits it for (model.py:379-382; the
    // LMM's per-variant extension); 2 the LMM as the reference has it -- ONE fit per block, of the block's last variant, given to every row
    // that passed (pyseer/lmm.py:209-213 calls fit_lineage_effect with the stale `k` of its loading loop)
    int lin_mode = 0;
    std::vector<std::string> lin_labels; std::vector<const char *> lin_ptrs;
    std::vector<int32_t> lin_host;
    // --output-patterns (sh_job_set_patterns): base64(md5) of every tested row, computed on the device (job_kernels.hip); the text of the block
    // last collected, until the next collect
    int patterns = 0;
    std::vector<char> pat_text; int64_t pat_n = 0;
    // --count-patterns (sh_job_set_pattern_count): the same rows go into the context's set of distinct patterns (patset_api.inc), no md5
    int pattern_count = 0;
    // --print-samples (sh_job_set_samples): the sample names in the order the reference lists them (sorted), for the printed rows' two lists
    std::string smp_blob; std::vector<int64_t> smp_off; std::vector<int32_t> smp_order;
};

static long long *slot_hdr(JobSlot &s) { return (long long *)s.h_res; }
static int32_t *slot_idx(JobSlot &s) { return (int32_t *)(s.h_res + 64); }
static uint32_t *slot_flags(JobSlot &s) { return (uint32_t *)(s.h_res + 64 + (size_t)s.cap_res_rows * 4); }
static double *slot_cols(JobSlot &s) { return (double *)(s.h_res + 64 + (size_t)s.cap_res_rows * 8); }
static int32_t *slot_lin(JobSlot &s) { return (int32_t *)(s.h_res + 64 + (size_t)s.cap_res_rows * (8 + 8 * (size_t)s.res_nrow)); }

static void job_free_slot(JobSlot &s)
{
    hipFree(s.d_bits); hipFree(s.d_out); hipFree(s.d_flags); hipFree(s.d_bcount); hipFree(s.d_hdr); hipFree(s.d_sel); hipFree(s.d_T1); hipFree(s.d_dig); hipFree(s.d_pat);
    if (s.h_pat) hipHostFree(s.h_pat);
    if (s.hp_bits) hipHostFree(s.hp_bits);
    if (s.h_res) hipHostFree(s.h_res);
    if (s.ev_h2d) hipEventDestroy(s.ev_h2d);
    if (s.ev_done) hipEventDestroy(s.ev_done);
    s = JobSlot();
}

static int job_ensure(sh_job *j, JobSlot &s, int64_t V, int64_t row_bytes, bool staged)
{
    const int nrow = j->nrow;
    if (V * row_bytes > s.cap_bits) { hipFree(s.d_bits); s.d_bits = nullptr; s.cap_bits = 0; HIPCHK(hipMalloc((void **)&s.d_bits, V * row_bytes)); s.cap_bits = V * row_bytes; }
    if (V > s.cap_rows || nrow > s.cap_nrow) {
        hipFree(s.d_out); hipFree(s.d_flags); hipFree(s.d_bcount); hipFree(s.d_hdr); s.d_out = nullptr; s.d_flags = nullptr; s.d_bcount = nullptr; s.d_hdr = nullptr; s.cap_rows = 0;
        const int64_t cv = std::max(V, s.cap_rows); const int cn = std::max(nrow, s.cap_nrow);
        HIPCHK(dmalloc(&s.d_out, (size_t)cv * cn)); HIPCHK(dmalloc(&s.d_flags, cv)); HIPCHK(dmalloc(&s.d_bcount, cv / JOB_ROWS_PER_BLOCK_HOST + 2)); HIPCHK(dmalloc(&s.d_hdr, 8));
        s.cap_rows = cv; s.cap_nrow = cn;
    }
    if (V > s.cap_res_rows || nrow > s.res_nrow) {
        if (s.h_res) hipHostFree(s.h_res);
        s.h_res = nullptr; s.cap_res_rows = 0;
        const int64_t cv = (std::max(V, s.cap_res_rows) + 15) / 16 * 16; const int cn = std::max(nrow, s.res_nrow);
        HIPCHK(hipHostMalloc((void **)&s.h_res, 64 + (size_t)cv * (8 + 8 * (size_t)cn + 4), hipHostMallocDefault));
        s.cap_res_rows = cv; s.res_nrow = cn;
    }
    if (j->lin_mode == 1 && V > s.cap_sel) { hipFree(s.d_sel); s.d_sel = nullptr; s.cap_sel = 0; HIPCHK(dmalloc(&s.d_sel, V)); s.cap_sel = V; }
    if (j->lin_mode == 2 && !s.d_T1) HIPCHK(dmalloc(&s.d_T1, (size_t)256 * j->c->NB64p));
    if (j->patterns && V > s.cap_pat) {
        hipFree(s.d_dig); hipFree(s.d_pat); if (s.h_pat) hipHostFree(s.h_pat);
        s.d_dig = nullptr; s.d_pat = nullptr; s.h_pat = nullptr; s.cap_pat = 0;
        HIPCHK(dmalloc(&s.d_dig, (size_t)V * 4)); HIPCHK(hipMalloc((void **)&s.d_pat, (size_t)V * 25));
        HIPCHK(hipHostMalloc((void **)&s.h_pat, (size_t)V * 25, hipHostMallocDefault)); s.cap_pat = V;
    }
    if (staged && V * row_bytes > s.cap_hp) {
        if (s.hp_bits) hipHostFree(s.hp_bits);
        s.hp_bits = nullptr; s.cap_hp = 0;
        HIPCHK(hipHostMalloc((void **)&s.hp_bits, V * row_bytes, hipHostMallocDefault)); s.cap_hp = V * row_bytes;
    }
    if (!s.ev_h2d) {
        HIPCHK(hipEventCreateWithFlags(&s.ev_h2d, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
    }
    return SH_OK;
}

// Wait for an event with the thread ASLEEP.  hipEventSynchronize and hipStreamSynchronize spin on this runtime whatever the event's flags
// (tools/ubench/host_feed_probe.hip, lines F0-F2 of profiles/r05/host_feed_probe.txt: CPU seconds = wall seconds, hipEventBlockingSync
// included), i.e. one CPU per waiting stream -- half of a 16-CPU quota with eight device streams.  A block takes milliseconds: the event is
// polled between sleeps that grow from 50 us to 1 ms (round 5 polled every 100 us: ~80 wake-ups per 8 ms block at ~10 us of system time
// each were half of a stream thread's CPU, profiles/r06/host_budget.json; the ring holds two more blocks, so collecting one up to a
// millisecond late leaves the device fed).
static int wait_event_asleep(hipEvent_t ev)
{
    long ns = 50000;
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return SH_OK;
        if (e != hipErrorNotReady) { (void)hipGetLastError(); return fail(SH_EHIP, std::string("hipEventQuery: ") + hipGetErrorString(e)); }
        struct timespec ts = {0, ns};
        nanosleep(&ts, nullptr);
        if (ns < 1000000) ns = std::min(1000000l, ns * 2);
    }
}

// the kernels of the block in slot s on context k (the job's own, or one of its lanes): the batch itself, then the sink's selection (job_kernels.hip)
static int job_compute_on(sh_job *j, JobSlot &s, sh_ctx *k)
{
    HIPCHK(hipStreamWaitEvent(k->stream, s.ev_h2d, 0));
    int rc = j->lmm ? sh_lmm_batch_dev(k, s.d_bits, s.row_bytes, s.V, s.d_out, s.d_flags) : sh_glm_batch_dev(k, s.d_bits, s.row_bytes, s.V, s.d_out, s.d_flags);
    if (rc) return rc;
    HIPCHK(shk_job_select(k->stream, s.d_flags, s.d_out, s.V, j->nrow, j->lmm, j->print_filtered, s.d_bcount, s.d_hdr, slot_hdr(s), slot_idx(s), slot_flags(s),
                          slot_cols(s), s.cap_res_rows, j->lin_mode == 1 ? s.d_sel : nullptr));
    if (j->pattern_count) {
        // the rows as submitted (the batch's own copy may be AF-compacted, de-duplicated or complemented), behind the flags they are chosen by
        rc = patset_insert_rows(j->c, k->stream, s.d_bits, s.row_bytes, s.V, s.d_flags); if (rc) return rc;
    }
    const int64_t Vpad = (s.V + 255) / 256 * 256;
    if (j->lin_mode == 1 || j->patterns) {
        // the block's rows repacked into this context's workspace, behind the batch that used it (whose own copy may be AF-compacted,
        // de-duplicated or complemented)
        rc = ensure_ws(k, Vpad); if (rc) return rc;
        HIPCHK(shk_repack_bits(k->stream, s.d_bits, s.row_bytes, s.V, Vpad, k->N, k->NB64p, k->d_T, nullptr));
    }
    if (j->patterns)
        HIPCHK(shk_job_patterns(k->stream, k->d_T, Vpad, s.V, k->N, s.d_flags, s.d_bcount, s.d_hdr + 4, s.d_dig, s.d_pat, s.h_pat));
    if (j->lin_mode) {
        // fit_lineage_effect (model.py:151-199) on the device, for rows the run prints: the design [1, lineages, covariates] is the parent
        // context's (sh_lineage_setup)
        const GlmState &pg = j->c->glm;
        if (j->lin_mode == 1) {
            const LinList L{s.d_sel, s.d_hdr, s.d_flags, j->lmm ? 2 : 1};
            HIPCHK(glm_lineage_launch(pg, k->stream, k->d_T, Vpad, s.V, k->N, k->NB64, slot_lin(s), L));
        } else {
            HIPCHK(shk_repack_bits(k->stream, s.d_bits + (s.V - 1) * s.row_bytes, s.row_bytes, 1, 256, k->N, k->NB64p, s.d_T1, nullptr));
            const LinList L{nullptr, nullptr, nullptr, 0};
            int *one = (int *)(slot_hdr(s) + 4);
            HIPCHK(glm_lineage_launch(pg, k->stream, s.d_T1, 256, 1, k->N, k->NB64, one, L));
        }
    }
    HIPCHK(hipEventRecord(s.ev_done, k->stream));
    return SH_OK;
}

static int job_compute(sh_job *j, JobSlot &s)
{
    sh_ctx *c = j->c;
    if (j->lanes > 1) {                                                 // fixed effects: on a lane, asynchronously
        int rc = lanes_ensure(c); if (rc) return rc;
        JobSlot *sp = &s;
        const double mn = c->min_af, mx = c->max_af; const int afon = c->af_on, dd = c->dedup;
        return lanes_push(c, [=](sh_ctx *k) -> int {
            shost::CpuScope cs(shost::ST_SUBMIT);
            k->min_af = mn; k->max_af = mx; k->af_on = afon; k->dedup = dd;
            const int rc2 = job_compute_on(j, *sp, k);
            {
                std::lock_guard<std::mutex> lk(j->mu);
                sp->state = rc2 ? 3 : 2; sp->rc = rc2; if (rc2) sp->err = g_err;
            }
            j->cv.notify_all();
            return rc2;
        });
    }
    shost::CpuScope cs(shost::ST_SUBMIT);
    const int rc = job_compute_on(j, s, c); if (rc) return rc;
    s.state = 2;
    return SH_OK;
}

sh_job *sh_job_open(sh_ctx *c, int lmm, int print_filtered)
{
    if (!c) { g_err = "null ctx"; return nullptr; }
    if (lmm ? !c->lmm_ready : !c->glm.ready) { g_err = "sh_job_open: the model of the job has not been set up on this context"; return nullptr; }
    if (hipSetDevice(c->device) != hipSuccess) { g_err = "hipSetDevice failed"; return nullptr; }
    sh_job *j = new sh_job();
    j->c = c; j->lmm = lmm ? 1 : 0; j->print_filtered = print_filtered ? 1 : 0;
    j->q = lmm ? 0 : c->glm.q; j->nrow = 5 + j->q;
    j->lanes = lmm ? 1 : std::max(1, std::min(c->n_lanes, 8));
    j->depth = j->lanes > 1 ? SH_JOB_DEPTH - 1 + j->lanes : SH_JOB_DEPTH;
    if (hipStreamCreateWithFlags(&j->copy_stream, hipStreamNonBlocking) != hipSuccess) { g_err = "hipStreamCreate failed"; delete j; return nullptr; }
    if (j->lanes > 1 && lanes_ensure(c) != SH_OK) { hipStreamDestroy(j->copy_stream); delete j; return nullptr; }   // (set up here, not under the first block)
    return j;
}

int sh_job_set_patterns(sh_job *j, int on)
{
    if (!j) return fail(SH_EINVAL, "null job");
    if (j->n_submitted != j->n_collected) return fail(SH_EINVAL, "sh_job_set_patterns: blocks are in flight");
    j->patterns = on ? 1 : 0;
    return SH_OK;
}

int sh_job_set_pattern_count(sh_job *j, int on)
{
    if (!j) return fail(SH_EINVAL, "null job");
    if (j->n_submitted != j->n_collected) return fail(SH_EINVAL, "sh_job_set_pattern_count: blocks are in flight");
    if (on && !j->c->patset) return fail(SH_EINVAL, "sh_job_set_pattern_count: sh_patset_begin has not run on the job's context");
    j->pattern_count = on ? 1 : 0;
    return SH_OK;
}

int sh_job_patterns(sh_job *j, const char **text, int64_t *nbytes)
{
    if (!j || !text || !nbytes) return fail(SH_EINVAL, "sh_job_patterns: null argument");
    *text = j->pat_text.data(); *nbytes = j->pat_n;
    return SH_OK;
}

int sh_job_set_samples(sh_job *j, const char *names, const int64_t *name_off, const int32_t *order, int n)
{
    if (!j || !names || !name_off || !order || n != j->c->N) return fail(SH_EINVAL, "sh_job_set_samples: one name per sample of the context, and their print order");
    if (j->n_submitted != j->n_collected) return fail(SH_EINVAL, "sh_job_set_samples: blocks are in flight");
    j->smp_blob.assign(names, names + name_off[n]); j->smp_off.assign(name_off, name_off + n + 1); j->smp_order.assign(order, order + n);
    for (int i = 0; i < n; ++i) if (order[i] < 0 || order[i] >= n) { j->smp_order.clear(); return fail(SH_EINVAL, "sh_job_set_samples: order out of range"); }
    return SH_OK;
}

int sh_job_set_lineage(sh_job *j, const char *const *labels, int n_labels, int per_variant)
{
    if (!j || !labels || n_labels < 1) return fail(SH_EINVAL, "sh_job_set_lineage: bad argument");
    if (!j->c->glm.lin_n) return fail(SH_EINVAL, "sh_job_set_lineage: sh_lineage_setup has not run on the job's context");
    if (n_labels != j->c->glm.lin_n) return fail(SH_EINVAL, "sh_job_set_lineage: one label per lineage column of sh_lineage_setup");
    if (j->n_submitted != j->n_collected) return fail(SH_EINVAL, "sh_job_set_lineage: blocks are in flight");
    j->lin_labels.assign(labels, labels + n_labels);
    j->lin_ptrs.clear();
    for (const std::string &l : j->lin_labels) j->lin_ptrs.push_back(l.c_str());
    j->lin_mode = (!j->lmm || per_variant) ? 1 : 2;
    return SH_OK;
}

void sh_job_close(sh_job *j)
{
    if (!j) return;
    hipSetDevice(j->c->device);
    (void)lanes_wait(j->c);                                             // (lane tasks hold pointers into the slots)
    hipStreamSynchronize(j->c->stream);
    if (j->copy_stream) { hipStreamSynchronize(j->copy_stream); hipStreamDestroy(j->copy_stream); }
    for (auto &s : j->slot) job_free_slot(s);
    delete j;
}

// The block's rows as ONE range of host memory (bits), or -- the library's own block loop over a packed cache whose stored blocks are smaller
// than the job's (job_run.inc) -- as n_seg ranges of whole rows that are DMA-able where they lie (seg_bits[i], seg_rows[i] rows each, V in
// all): every range is copied to its place in the slot's device buffer by the copy engine, nothing is gathered on the host.
static int job_submit_rows(sh_job *j, const uint8_t *bits, const uint8_t *const *seg_bits, const int64_t *seg_rows, int n_seg, int64_t row_bytes, int64_t V,
                           const int32_t *counts, const char *names, const int64_t *name_off, int rows_are_dma)
{
    if (!j) return fail(SH_EINVAL, "null job");
    if ((!bits && n_seg <= 0) || !counts || !names || !name_off || V <= 0 || row_bytes <= 0) return fail(SH_EINVAL, "sh_job_submit: bad argument");
    if (n_seg > 0) {
        int64_t sum = 0;
        for (int i = 0; i < n_seg; ++i) { if (!seg_bits[i] || seg_rows[i] <= 0) return fail(SH_EINVAL, "sh_job_submit: bad segment"); sum += seg_rows[i]; }
        if (sum != V || !rows_are_dma) return fail(SH_EINVAL, "sh_job_submit: the segments must be DMA-able and hold V rows in all");
        if (!j->smp_order.empty()) return fail(SH_EINVAL, "sh_job_submit: --print-samples reads the block's rows on the host: one range");
    }
    if (row_bytes * 8 < j->c->N) return fail(SH_ESHAPE, "row_bytes*8 < n_samples: shape mismatch between snps and Y");
    if (j->n_submitted - j->n_collected >= (uint64_t)j->depth) return fail(SH_EINVAL, "sh_job_submit: every slot holds a block; collect one first");
    sh_ctx *c = j->c;
    HIPCHK(hipSetDevice(c->device));
    JobSlot &s = j->slot[j->n_submitted % j->depth];
    int rc = job_ensure(j, s, V, row_bytes, !rows_are_dma); if (rc) return rc;
    s.bits = bits; s.row_bytes = row_bytes; s.V = V; s.counts = counts; s.names = names; s.name_off = name_off;
    // rows -> device on the copy stream.  DMA-able where they lie (pinned or registered: the packed-cache mapping): nothing but the descriptor
    // is touched by the CPU.  Otherwise through this slot's pinned slab, filled by the caller and the idle workers of the process-wide pool.
    const uint8_t *src = bits;
    if (!rows_are_dma) {
        shost::CpuScope cs(shost::ST_STAGE_COPY);
        const size_t nbytes = (size_t)(V * row_bytes), piece = (size_t)4 << 20, np = (nbytes + piece - 1) / piece;
        uint8_t *dst = s.hp_bits;
        const std::function<void(int64_t)> cp = [&](int64_t i) { const size_t lo = (size_t)i * piece, hi = std::min(nbytes, lo + piece); std::memcpy(dst + lo, bits + lo, hi - lo); };
        shost::pool().run((int64_t)np, 1, cp, shost::ST_STAGE_COPY, shost::per_stream_cpus(2));
        src = s.hp_bits;
    }
    {
        shost::CpuScope cs(shost::ST_SUBMIT);
        if (n_seg > 0) {
            size_t at = 0;
            for (int i = 0; i < n_seg; ++i) {
                HIPCHK(hipMemcpyAsync(s.d_bits + at, seg_bits[i], (size_t)(seg_rows[i] * row_bytes), hipMemcpyHostToDevice, j->copy_stream));
                at += (size_t)(seg_rows[i] * row_bytes);
            }
        } else
            HIPCHK(hipMemcpyAsync(s.d_bits, src, (size_t)(V * row_bytes), hipMemcpyHostToDevice, j->copy_stream));
        HIPCHK(hipEventRecord(s.ev_h2d, j->copy_stream));
    }
    s.state = 1;
    ++j->n_submitted;
    // On the lanes (fixed effects) the block's kernels are handed over at once: the lane's stream waits for the upload on the device, and a
    // lane that finishes takes the next block from the queue without this thread's help (handing block k over only at the submit of k + 1
    // left a finished lane idle for a collect + format + read + submit of the caller: the device stood idle 18-28 % of a job).
    // Without lanes: the kernels of the block BEFORE this one -- its rows have had a whole block's time to arrive, and the launch code
    // (which blocks on its read-backs) runs with this block's upload already in flight.
    while (j->n_computed + (j->lanes > 1 ? 0 : 1) < j->n_submitted) {
        rc = job_compute(j, j->slot[j->n_computed % j->depth]); if (rc) return rc;
        ++j->n_computed;
    }
    return SH_OK;
}

int sh_job_submit(sh_job *j, const uint8_t *bits, int64_t row_bytes, int64_t V, const int32_t *counts, const char *names, const int64_t *name_off, int rows_are_dma)
{
    if (!bits) return fail(SH_EINVAL, "sh_job_submit: bad argument");
    return job_submit_rows(j, bits, nullptr, nullptr, 0, row_bytes, V, counts, names, name_off, rows_are_dma);
}

int64_t sh_job_pending(sh_job *j) { return j ? (int64_t)(j->n_submitted - j->n_collected) : 0; }
int sh_job_depth(sh_job *j) { return j ? j->depth : 0; }

int sh_job_collect(sh_job *j, const char **text, int64_t *nbytes, int64_t *counters)
{
    if (!j || !text || !nbytes || !counters) return fail(SH_EINVAL, "sh_job_collect: null argument");
    if (j->n_collected >= j->n_submitted) return fail(SH_EINVAL, "sh_job_collect: nothing submitted");
    sh_ctx *c = j->c;
    HIPCHK(hipSetDevice(c->device));
    while (j->n_computed <= j->n_collected) {                           // (the last block of a stream: nobody submitted after it)
        int rc = job_compute(j, j->slot[j->n_computed % j->depth]); if (rc) return rc;
        ++j->n_computed;
    }
    JobSlot &s = j->slot[j->n_collected % j->depth];
    if (j->lanes > 1) {                                                 // the lane has queued the block's kernels (or failed)
        std::unique_lock<std::mutex> lk(j->mu);
        j->cv.wait(lk, [&] { return s.state >= 2; });
        if (s.state == 3) { const int e = s.rc; const std::string m = s.err; s.state = 0; ++j->n_collected; lk.unlock(); (void)lanes_wait(c); return fail(e, "lane: " + m); }
    }
    {
        shost::CpuScope cs(shost::ST_COLLECT);
        const int rcw = wait_event_asleep(s.ev_done); if (rcw) return rcw;
    }
    const long long nsel = slot_hdr(s)[0], npf = slot_hdr(s)[1];
    if (nsel < 0 || nsel > s.V || npf < 0 || npf > s.V) return fail(SH_EHIP, "sh_job_collect: the device left an impossible count");
    counters[0] = npf; counters[1] = s.V - npf; counters[2] = nsel;
    *text = ""; *nbytes = 0;
    j->pat_n = 0;
    if (j->patterns) {                                                  // (the slot's pinned text may be overwritten by the block that takes the slot next)
        j->pat_n = 25 * (s.V - npf);
        if ((int64_t)j->pat_text.size() < j->pat_n) j->pat_text.resize((size_t)j->pat_n);
        std::memcpy(j->pat_text.data(), s.h_pat, (size_t)j->pat_n);
    }
    if (nsel > 0) {
        const double *cols[5]; for (int a = 0; a < 5; ++a) cols[a] = slot_cols(s) + (size_t)a * (size_t)s.cap_res_rows;
        const double *betas = j->q > 0 ? slot_cols(s) + (size_t)5 * (size_t)s.cap_res_rows : nullptr;
        if (j->q > 0) {                                                 // utils.py:86-91 prints the slopes of a variant that was fitted
            j->valid.resize((size_t)nsel);
            const double *pv = cols[1], *kb = cols[2];
            for (long long r = 0; r < nsel; ++r) j->valid[(size_t)r] = (std::isfinite(kb[r]) || std::isfinite(pv[r])) ? 1 : 0;
        }
        const int32_t *lin = nullptr;
        if (j->lin_mode == 1) lin = slot_lin(s);
        else if (j->lin_mode == 2) {                                    // the block's one fit, for the rows that passed (lmm.py:200-213)
            const int32_t ml = *(const int32_t *)(slot_hdr(s) + 4);
            const uint32_t *fl = slot_flags(s);
            j->lin_host.resize((size_t)nsel);
            for (long long r = 0; r < nsel; ++r) j->lin_host[(size_t)r] = (fl[r] & (SH_FLAG_PREFILTER | SH_FLAG_FILTER)) ? -1 : ml;
            lin = j->lin_host.data();
        }
        const int64_t n = format_records_samples(s.names, s.name_off, s.counts, c->N, slot_idx(s), nsel, cols, 5, betas, s.cap_res_rows, j->q,
                                            j->q > 0 ? j->valid.data() : nullptr, lin, lin ? j->lin_ptrs.data() : nullptr, (int)j->lin_ptrs.size(),
                                            slot_flags(s), text, j->smp_order.empty() ? nullptr : s.bits, s.row_bytes, j->smp_blob.data(), j->smp_off.data(),
                                            j->smp_order.data());
        if (n < 0) return fail(SH_EINVAL, "sh_format_records failed");
        *nbytes = n;
    }
    s.state = 0;
    ++j->n_collected;
    return SH_OK;
}

// ---- host memory the device may read by DMA where it lies (the packed-cache mapping) -------------------------------------------------------
int sh_host_register(const void *p, int64_t nbytes, int device)
{
    if (!p || nbytes <= 0) return fail(SH_EINVAL, "sh_host_register: bad argument");
    shost::CpuScope cs(shost::ST_REGISTER);
    HIPCHK(hipSetDevice(device));                                       // (the calling thread is usually a reader thread that has not chosen one)
    const uintptr_t pg = 4096, lo = (uintptr_t)p & ~(pg - 1), hi = ((uintptr_t)p + (uintptr_t)nbytes + pg - 1) & ~(pg - 1);
    const hipError_t e = hipHostRegister((void *)lo, hi - lo, hipHostRegisterDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(SH_EHIP, std::string("hipHostRegister: ") + hipGetErrorString(e)); }
    return SH_OK;
}

int sh_host_unregister(const void *p)
{
    if (!p) return fail(SH_EINVAL, "sh_host_unregister: null");
    shost::CpuScope cs(shost::ST_REGISTER);
    const uintptr_t pg = 4096, lo = (uintptr_t)p & ~(pg - 1);
    const hipError_t e = hipHostUnregister((void *)lo);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(SH_EHIP, std::string("hipHostUnregister: ") + hipGetErrorString(e)); }
    return SH_OK;
}

// ---- the host CPU budget (host_pool.h) -------------------------------------------------------------------------------------------------------
int sh_host_cpus(void) { return shost::host_cpus(); }
void sh_set_host_threads(int n) { shost::cpus_override().store(n > 0 ? n : 0); }
void sh_set_host_streams(int n) { shost::streams().store(n < 1 ? 1 : n); }
int sh_host_pool_workers(void) { return shost::pool().workers(); }
// thread CPU seconds spent so far in each host stage of the library, as "name=seconds" items joined by ',' (tools/gpu_e2e_job.py)
int sh_host_cpu_seconds(char *buf, int cap)
{
    std::string s;
    for (int i = 0; i < shost::ST_COUNT; ++i) {
        char t[64]; snprintf(t, sizeof t, "%s%s=%.6f", i ? "," : "", shost::kStageName[i], (double)shost::stage_ns()[i].load() * 1e-9);
        s += t;
    }
    if (!buf || cap <= (int)s.size()) return -(int)s.size() - 1;
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return (int)s.size();
}
