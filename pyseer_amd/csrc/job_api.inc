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
    // a call block (sh_job_submit_calls): d_bits holds [present | missing | n_present, n_missing, skip] (calls_layout), miss: the caller's missing plane
    // (--print-samples), cnt_host: present + missing per row (the printed af), no_last_lineage: the block's last row was skipped or holds a missing call
    int calls = 0, no_last_lineage = 0; const uint8_t *miss = nullptr; double max_missing = 0.0; std::vector<int32_t> cnt_host;
    // a call block selected on the device (sh_job_submit_calls_select, select_api.inc): the counts are k_calls_select's and lie in the pinned slab
    // once ev_done has passed -- cnt_host and no_last_lineage are made from them at the collect
    int counts_from_device = 0;
    uint32_t *d_flags_rows = nullptr; int64_t cap_frows = 0;            // --count-patterns: the flags by which the pattern set takes packed rows
    int64_t cap_dig = 0;
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
    // sh_job_set_calls_timing: stream events around k_job_calls_mark [0] and k_job_md5_calls [1] of every call block (recorded by whichever
    // thread queues the block's kernels: under mu)
    int time_calls = 0; std::vector<std::pair<hipEvent_t, hipEvent_t>> tev_calls[2];
};

// one kernel launch between two events on st, kept in j->tev_calls[which] (sh_job_calls_times)
static int job_timed(sh_job *j, int which, hipStream_t st, const std::function<hipError_t()> &launch)
{
    if (!j->time_calls) { HIPCHK(launch()); return SH_OK; }
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
    HIPCHK(hipEventRecord(a, st));
    const hipError_t e = launch();
    HIPCHK(hipEventRecord(b, st));
    { std::lock_guard<std::mutex> lk(j->mu); j->tev_calls[which].emplace_back(a, b); }
    HIPCHK(e);
    return SH_OK;
}

static long long *slot_hdr(JobSlot &s) { return (long long *)s.h_res; }
static int32_t *slot_idx(JobSlot &s) { return (int32_t *)(s.h_res + 64); }
static uint32_t *slot_flags(JobSlot &s) { return (uint32_t *)(s.h_res + 64 + (size_t)s.cap_res_rows * 4); }
static double *slot_cols(JobSlot &s) { return (double *)(s.h_res + 64 + (size_t)s.cap_res_rows * 8); }
static int32_t *slot_lin(JobSlot &s) { return (int32_t *)(s.h_res + 64 + (size_t)s.cap_res_rows * (8 + 8 * (size_t)s.res_nrow)); }

// where the parts of a call block lie in the slot's device buffer (and in its pinned slab)
struct CallsLayout { size_t miss, ints, total; };
static CallsLayout calls_layout(int64_t V, int64_t row_bytes)
{
    CallsLayout L; L.miss = (size_t)(V * row_bytes); L.ints = (2 * L.miss + 15) / 16 * 16; L.total = L.ints + (size_t)V * 12;
    return L;
}

static void job_free_slot(JobSlot &s)
{
    hipFree(s.d_flags_rows);
    hipFree(s.d_bits); hipFree(s.d_out); hipFree(s.d_flags); hipFree(s.d_bcount); hipFree(s.d_hdr); hipFree(s.d_sel); hipFree(s.d_T1); hipFree(s.d_dig); hipFree(s.d_pat);
    if (s.h_pat) hipHostFree(s.h_pat);
    if (s.hp_bits) hipHostFree(s.hp_bits);
    if (s.h_res) hipHostFree(s.h_res);
    if (s.ev_h2d) hipEventDestroy(s.ev_h2d);
    if (s.ev_done) hipEventDestroy(s.ev_done);
    s = JobSlot();
}

static int job_ensure(sh_job *j, JobSlot &s, int64_t V, int64_t row_bytes, bool staged, bool calls = false)
{
    const int nrow = j->nrow;
    const int64_t nbits = calls ? (int64_t)calls_layout(V, row_bytes).total : V * row_bytes;
    if (nbits > s.cap_bits) { hipFree(s.d_bits); s.d_bits = nullptr; s.cap_bits = 0; HIPCHK(hipMalloc((void **)&s.d_bits, nbits)); s.cap_bits = nbits; }
    if (calls && j->pattern_count && V > s.cap_frows) { hipFree(s.d_flags_rows); s.d_flags_rows = nullptr; s.cap_frows = 0; HIPCHK(dmalloc(&s.d_flags_rows, V)); s.cap_frows = V; }
    if ((j->patterns || (calls && j->pattern_count)) && V > s.cap_dig) { hipFree(s.d_dig); s.d_dig = nullptr; s.cap_dig = 0; HIPCHK(dmalloc(&s.d_dig, (size_t)V * 4)); s.cap_dig = V; }
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
        hipFree(s.d_pat); if (s.h_pat) hipHostFree(s.h_pat);
        s.d_pat = nullptr; s.h_pat = nullptr; s.cap_pat = 0;
        HIPCHK(hipMalloc((void **)&s.d_pat, (size_t)V * 25));
        HIPCHK(hipHostMalloc((void **)&s.h_pat, (size_t)V * 25, hipHostMallocDefault)); s.cap_pat = V;
    }
    if (staged && nbits > s.cap_hp) {
        if (s.hp_bits) hipHostFree(s.hp_bits);
        s.hp_bits = nullptr; s.cap_hp = 0;
        HIPCHK(hipHostMalloc((void **)&s.hp_bits, nbits, hipHostMallocDefault)); s.cap_hp = nbits;
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
    const CallsLayout CL = calls_layout(s.V, s.row_bytes);
    const uint8_t *d_miss = s.calls ? s.d_bits + CL.miss : nullptr;
    const int32_t *d_np = s.calls ? (const int32_t *)(s.d_bits + CL.ints) : nullptr, *d_nm = s.calls ? d_np + s.V : nullptr, *d_skip = s.calls ? d_nm + s.V : nullptr;
    if (s.calls) {
        // skipped records, rows outside the filters and rows with missing calls, per submitted row (k_job_calls_mark, job_kernels.hip); the
        // phenotype masks and the centred phenotype are those of the context that ran the batch
        const bool lm = j->lmm != 0;
        rc = job_timed(j, 0, k->stream, [&] {
            return shk_job_calls_mark(k->stream, s.d_bits, d_miss, s.row_bytes, s.V, d_np, d_nm, d_skip, lm ? k->d_y1 : k->glm.d_y1, lm ? k->d_y0 : k->glm.d_y0,
                                      lm ? k->d_yc : k->glm.d_yc, k->N, j->lmm, lm ? k->fin.continuous : k->glm.P.continuous, j->nrow, k->min_af, k->max_af,
                                      s.max_missing, lm ? k->fin.pret : k->glm.P.pret, s.d_out, s.d_flags, j->pattern_count ? s.d_flags_rows : nullptr); });
        if (rc) return rc;
    }
    HIPCHK(shk_job_select(k->stream, s.d_flags, s.d_out, s.V, j->nrow, j->lmm, j->print_filtered, s.d_bcount, s.d_hdr, slot_hdr(s), slot_idx(s), slot_flags(s),
                          slot_cols(s), s.cap_res_rows, j->lin_mode == 1 ? s.d_sel : nullptr));
    if (j->pattern_count) {
        // the rows as submitted (the batch's own copy may be AF-compacted, de-duplicated or complemented), behind the flags they are chosen by
        // (a call block's rows with missing calls are no packed rows: they enter as md5 digests below)
        rc = patset_insert_rows(j->c, k->stream, s.d_bits, s.row_bytes, s.V, s.calls ? s.d_flags_rows : s.d_flags); if (rc) return rc;
    }
    const int64_t Vpad = (s.V + 255) / 256 * 256;
    if (j->lin_mode == 1 || j->patterns) {
        // the block's rows repacked into this context's workspace, behind the batch that used it (whose own copy may be AF-compacted,
        // de-duplicated or complemented)
        rc = ensure_ws(k, Vpad); if (rc) return rc;
        HIPCHK(shk_repack_bits(k->stream, s.d_bits, s.row_bytes, s.V, Vpad, k->N, k->NB64p, k->d_T, nullptr));
    }
    if (j->patterns)
        HIPCHK(shk_job_patterns(k->stream, k->d_T, Vpad, s.V, k->N, s.d_flags, s.d_bcount, s.d_hdr + 4, s.d_dig, s.d_pat, s.h_pat, s.d_bits, d_miss, s.row_bytes, d_nm));
    else if (s.calls && j->pattern_count) {
        rc = job_timed(j, 1, k->stream, [&] { return shk_job_md5_calls(k->stream, s.d_bits, d_miss, s.row_bytes, s.V, k->N, s.d_flags, d_nm, s.d_dig); });
        if (rc) return rc;
    }
    if (s.calls && j->pattern_count) { rc = patset_insert_digests(j->c, k->stream, s.d_dig, s.V, s.d_flags, d_nm); if (rc) return rc; }
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

int sh_job_set_calls_timing(sh_job *j, int on)
{
    if (!j) return fail(SH_EINVAL, "null job");
    if (j->n_submitted != j->n_collected) return fail(SH_EINVAL, "sh_job_set_calls_timing: blocks are in flight");
    j->time_calls = on ? 1 : 0;
    return SH_OK;
}

// the sum of the recorded launches so far (and their number), after waiting for them; the record starts again
int sh_job_calls_times(sh_job *j, double *mark_ms, int64_t *mark_launches, double *md5_ms, int64_t *md5_launches)
{
    if (!j || !mark_ms || !mark_launches || !md5_ms || !md5_launches) return fail(SH_EINVAL, "sh_job_calls_times: null argument");
    if (j->n_submitted != j->n_collected) return fail(SH_EINVAL, "sh_job_calls_times: blocks are in flight");
    HIPCHK(hipSetDevice(j->c->device));
    double ms[2] = {0.0, 0.0}; int64_t n[2] = {0, 0};
    std::lock_guard<std::mutex> lk(j->mu);
    for (int w = 0; w < 2; ++w) {
        for (auto &pr : j->tev_calls[w]) {
            float t = 0.0f;
            HIPCHK(hipEventSynchronize(pr.second)); HIPCHK(hipEventElapsedTime(&t, pr.first, pr.second));
            hipEventDestroy(pr.first); hipEventDestroy(pr.second);
            ms[w] += (double)t; ++n[w];
        }
        j->tev_calls[w].clear();
    }
    *mark_ms = ms[0]; *mark_launches = n[0]; *md5_ms = ms[1]; *md5_launches = n[1];
    return SH_OK;
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
    for (auto &v : j->tev_calls) for (auto &pr : v) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
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
    s.calls = 0; s.miss = nullptr; s.no_last_lineage = 0; s.counts_from_device = 0;
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

// A block of calls as the native VCF / Rtab readers deliver them (round 20): the two packed planes, their counts and the reader's skip reason per
// record.  Every row is fitted from `present` by the batch; k_job_calls_mark then restates, per submitted row, what the reference does with
// skipped records, with rows outside the AF window (the context's: sh_set_af_filter) or above max_missing, and with rows that hold a missing
// call.  The planes and the counts go through the slot's pinned slab in one upload.
int sh_job_submit_calls(sh_job *j, const uint8_t *present, const uint8_t *missing, int64_t row_bytes, int64_t V, const int32_t *n_present, const int32_t *n_missing,
                        const int32_t *skip, const char *names, const int64_t *name_off, double max_missing)
{
    if (!j) return fail(SH_EINVAL, "null job");
    if (!present || !missing || !n_present || !n_missing || !skip || !names || !name_off || V <= 0 || row_bytes <= 0) return fail(SH_EINVAL, "sh_job_submit_calls: bad argument");
    if (row_bytes * 8 < j->c->N) return fail(SH_ESHAPE, "row_bytes*8 < n_samples: shape mismatch between snps and Y");
    if (j->n_submitted - j->n_collected >= (uint64_t)j->depth) return fail(SH_EINVAL, "sh_job_submit_calls: every slot holds a block; collect one first");
    for (int64_t v = 0; v < V; ++v)
        if (n_present[v] < 0 || n_missing[v] < 0 || (int64_t)n_present[v] + n_missing[v] > (int64_t)row_bytes * 8) return fail(SH_EINVAL, "sh_job_submit_calls: impossible counts");
    sh_ctx *c = j->c;
    HIPCHK(hipSetDevice(c->device));
    JobSlot &s = j->slot[j->n_submitted % j->depth];
    int rc = job_ensure(j, s, V, row_bytes, true, true); if (rc) return rc;
    s.bits = present; s.miss = missing; s.row_bytes = row_bytes; s.V = V; s.names = names; s.name_off = name_off;
    s.calls = 1; s.counts_from_device = 0; s.max_missing = max_missing; s.no_last_lineage = (skip[V - 1] != 0 || n_missing[V - 1] != 0) ? 1 : 0;
    s.cnt_host.resize((size_t)V);
    for (int64_t v = 0; v < V; ++v) s.cnt_host[(size_t)v] = n_present[v] + n_missing[v];   // the printed af: (present + missing) / N (input.py:446)
    s.counts = s.cnt_host.data();
    const CallsLayout CL = calls_layout(V, row_bytes);
    {
        shost::CpuScope cs(shost::ST_STAGE_COPY);
        std::memcpy(s.hp_bits, present, CL.miss); std::memcpy(s.hp_bits + CL.miss, missing, CL.miss);
        if (CL.ints > 2 * CL.miss) std::memset(s.hp_bits + 2 * CL.miss, 0, CL.ints - 2 * CL.miss);
        int32_t *ints = (int32_t *)(s.hp_bits + CL.ints);
        std::memcpy(ints, n_present, (size_t)V * 4); std::memcpy(ints + V, n_missing, (size_t)V * 4); std::memcpy(ints + 2 * V, skip, (size_t)V * 4);
    }
    {
        shost::CpuScope cs(shost::ST_SUBMIT);
        HIPCHK(hipMemcpyAsync(s.d_bits, s.hp_bits, CL.total, hipMemcpyHostToDevice, j->copy_stream));
        HIPCHK(hipEventRecord(s.ev_h2d, j->copy_stream));
    }
    s.state = 1;
    ++j->n_submitted;
    while (j->n_computed + (j->lanes > 1 ? 0 : 1) < j->n_submitted) {    // (as sh_job_submit hands the blocks' kernels over)
        rc = job_compute(j, j->slot[j->n_computed % j->depth]); if (rc) return rc;
        ++j->n_computed;
    }
    return SH_OK;
}

// the compacted records of the block last collected, as the device left them (what the text was formatted from): for callers that want the
// numbers and the flags of the printed rows, not their text.  Valid until the next submit.
int sh_job_records(sh_job *j, int64_t *nsel, const int32_t **idx, const uint32_t **flags, const double **cols, int64_t *stride, int *nrow)
{
    if (!j || !nsel || !idx || !flags || !cols || !stride || !nrow) return fail(SH_EINVAL, "sh_job_records: null argument");
    if (j->n_collected == 0) return fail(SH_EINVAL, "sh_job_records: nothing collected");
    JobSlot &s = j->slot[(j->n_collected - 1) % j->depth];
    *nsel = slot_hdr(s)[0]; *idx = slot_idx(s); *flags = slot_flags(s); *cols = slot_cols(s); *stride = s.cap_res_rows; *nrow = j->nrow;
    return SH_OK;
}

// n_present and n_missing of every row of the call block last collected, as its slot's pinned slab holds them: the caller's own for
// sh_job_submit_calls, k_calls_select's for sh_job_submit_calls_select.  Valid until the next submit.
int sh_job_calls_counts(sh_job *j, int64_t *V, const int32_t **n_present, const int32_t **n_missing)
{
    if (!j || !V || !n_present || !n_missing) return fail(SH_EINVAL, "sh_job_calls_counts: null argument");
    if (j->n_collected == 0) return fail(SH_EINVAL, "sh_job_calls_counts: nothing collected");
    JobSlot &s = j->slot[(j->n_collected - 1) % j->depth];
    if (!s.calls) return fail(SH_EINVAL, "sh_job_calls_counts: the block last collected was no call block");
    const int32_t *ints = (const int32_t *)(s.hp_bits + calls_layout(s.V, s.row_bytes).ints);
    *V = s.V; *n_present = ints; *n_missing = ints + s.V;
    return SH_OK;
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
    if (s.counts_from_device) {                                         // (the slab's counts came back on the selector's stream, which ev_done is behind)
        const int32_t *np_ = (const int32_t *)(s.hp_bits + calls_layout(s.V, s.row_bytes).ints), *nm_ = np_ + s.V;
        for (int64_t v = 0; v < s.V; ++v) s.cnt_host[(size_t)v] = np_[v] + nm_[v];
        if (nm_[s.V - 1] != 0) s.no_last_lineage = 1;
        s.counts_from_device = 0;
    }
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
            // (a call block whose last variant was skipped or holds a missing call has no lineage: cli_run.last_variant_lineage)
            const int32_t ml = s.no_last_lineage ? -1 : *(const int32_t *)(slot_hdr(s) + 4);
            const uint32_t *fl = slot_flags(s);
            j->lin_host.resize((size_t)nsel);
            for (long long r = 0; r < nsel; ++r) j->lin_host[(size_t)r] = (fl[r] & (SH_FLAG_PREFILTER | SH_FLAG_FILTER)) ? -1 : ml;
            lin = j->lin_host.data();
        }
        const int64_t n = format_records_samples(s.names, s.name_off, s.counts, c->N, slot_idx(s), nsel, cols, 5, betas, s.cap_res_rows, j->q,
                                            j->q > 0 ? j->valid.data() : nullptr, lin, lin ? j->lin_ptrs.data() : nullptr, (int)j->lin_ptrs.size(),
                                            slot_flags(s), text, j->smp_order.empty() ? nullptr : s.bits, s.row_bytes, j->smp_blob.data(), j->smp_off.data(),
                                            j->smp_order.data(), j->smp_order.empty() ? nullptr : s.miss);
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
