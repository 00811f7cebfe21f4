// patset_api.inc -- the run-wide set of distinct presence patterns of a context (included by api.hip inside its extern "C" block, before
// job_api.inc; kernels: patset_kernels.hip, the key: patset_hash.h).
//
// What it replaces: scripts/count_patterns.py of the reference (`LC_ALL=C sort -u patterns | wc -l`, then alpha / count) over the file that
// --output-patterns wrote: minutes of CPU sort over 25 bytes per tested variant, after a run of seconds.  The set is owned by the context
// and fed by whoever holds rows or keys: the job stream (sh_job_set_pattern_count: the rows k_job_md5 would digest, on the stream of the
// block's own kernels -- a lane's stream for a fixed-effects job), or the host (rows: sh_patset_add_rows; ready-made 128-bit keys such as md5
// digests: sh_patset_add_keys).
//
// Growth keeps the load at or below 1/2: before an insert is queued, slots >= 2 (upper bound of the distinct keys so far + the rows of this
// insert).  The bound is the host's sum of inserted rows, replaced by the device's count whenever that is read (sh_patset_count, and at a
// growth, which has waited for every insert anyway).  A growth waits for the inserts in flight on EVERY stream that fed the set (one event
// per queued insert), re-inserts the stored pairs into a table of the next sufficient power of two with k_ps_rehash, waits for that, and
// frees the old table; inserts from other threads (lanes) are held off by the set's mutex meanwhile.
struct PatSet {
    unsigned long long *k1 = nullptr, *k2 = nullptr, *cnt = nullptr;   // cnt[0]: distinct keys; cnt[1]: a probe sequence ran through the whole table
    int64_t slots = 0, ub = 0, growths = 0;
    std::mutex mu;                                                      // lanes queue inserts side by side
    std::deque<hipEvent_t> inflight;                                    // one per queued insert, reaped once complete
    uint8_t *d_stage = nullptr; int64_t cap_stage = 0;                  // host rows / keys on their way (the context's stream)
};

static int patset_table(int64_t slots, hipStream_t st, unsigned long long **k1, unsigned long long **k2)
{
    *k1 = *k2 = nullptr;
    if (hipMalloc((void **)k1, (size_t)slots * 8) != hipSuccess || hipMalloc((void **)k2, (size_t)slots * 8) != hipSuccess) {
        (void)hipGetLastError(); hipFree(*k1); *k1 = nullptr;
        return fail(SH_ENOMEM, "pattern set: no device memory for a table of " + std::to_string(slots) + " slots");
    }
    HIPCHK(hipMemsetAsync(*k1, 0xFF, (size_t)slots * 8, st));
    HIPCHK(hipMemsetAsync(*k2, 0xFF, (size_t)slots * 8, st));
    return SH_OK;
}

// every insert queued so far has completed (ps->mu held)
static int patset_drain(PatSet *ps)
{
    while (!ps->inflight.empty()) {
        const hipError_t e = hipEventSynchronize(ps->inflight.front());
        hipEventDestroy(ps->inflight.front()); ps->inflight.pop_front();
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(SH_EHIP, std::string("pattern set: hipEventSynchronize: ") + hipGetErrorString(e)); }
    }
    return SH_OK;
}

// the device's two words, after a drain; the count becomes the bound (ps->mu held)
static int patset_read(PatSet *ps, unsigned long long *h)
{
    HIPCHK(hipMemcpy(h, ps->cnt, 16, hipMemcpyDeviceToHost));
    if (h[1]) return fail(SH_EHIP, "pattern set: a probe sequence ran through the whole table (the load bound was broken)");
    ps->ub = (int64_t)h[0];
    return SH_OK;
}

// room for `add` more keys before their insert is queued on st (ps->mu held)
static int patset_reserve(PatSet *ps, hipStream_t st, int64_t add)
{
    if (2 * (ps->ub + add) <= ps->slots) return SH_OK;
    int rc = patset_drain(ps); if (rc) return rc;                       // inserts in flight on every stream that feeds the set
    unsigned long long h[2];
    rc = patset_read(ps, h); if (rc) return rc;
    const int64_t need = 2 * (ps->ub + add);
    if (need <= ps->slots) return SH_OK;
    int64_t ns = ps->slots;
    while (ns < need) ns *= 2;
    unsigned long long *n1, *n2;
    rc = patset_table(ns, st, &n1, &n2); if (rc) return rc;
    hipError_t e = shk_ps_rehash(st, ps->k1, ps->k2, ps->slots, n1, n2, ns, ps->cnt);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                  // (the next insert may come on another stream)
    if (e != hipSuccess) { hipFree(n1); hipFree(n2); return fail(SH_EHIP, std::string("pattern set: growth: ") + hipGetErrorString(e)); }
    hipFree(ps->k1); hipFree(ps->k2);
    ps->k1 = n1; ps->k2 = n2; ps->slots = ns; ++ps->growths;
    return SH_OK;
}

// an insert has been queued on st (ps->mu held)
static int patset_mark(PatSet *ps, hipStream_t st)
{
    while (!ps->inflight.empty() && hipEventQuery(ps->inflight.front()) == hipSuccess) { hipEventDestroy(ps->inflight.front()); ps->inflight.pop_front(); }
    (void)hipGetLastError();                                            // (hipErrorNotReady of the query)
    hipEvent_t ev;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    const hipError_t e = hipEventRecord(ev, st);
    if (e != hipSuccess) { hipEventDestroy(ev); return fail(SH_EHIP, std::string("pattern set: hipEventRecord: ") + hipGetErrorString(e)); }
    ps->inflight.push_back(ev);
    return SH_OK;
}

// rows on the device into the set of context c, on stream st (c's own, or one of its lanes'); flags: rows with SH_FLAG_PREFILTER are left out
static int patset_insert_rows(sh_ctx *c, hipStream_t st, const uint8_t *d_bits, int64_t row_bytes, int64_t V, const uint32_t *d_flags)
{
    PatSet *ps = c->patset;
    if (!ps) return fail(SH_EINVAL, "pattern set: sh_patset_begin has not run on this context");
    if (V <= 0) return SH_OK;
    std::lock_guard<std::mutex> lk(ps->mu);
    const int rc = patset_reserve(ps, st, V); if (rc) return rc;
    HIPCHK(shk_ps_insert_rows(st, d_bits, row_bytes, V, c->N, d_flags, ps->k1, ps->k2, ps->slots, ps->cnt));
    ps->ub += V;
    return patset_mark(ps, st);
}

// md5 digests on the device (four words per row) of the rows that are tested and hold a missing call (job_api.inc: call blocks), on stream st
static int patset_insert_digests(sh_ctx *c, hipStream_t st, const uint32_t *d_digest, int64_t V, const uint32_t *d_flags, const int32_t *d_n_missing)
{
    PatSet *ps = c->patset;
    if (!ps) return fail(SH_EINVAL, "pattern set: sh_patset_begin has not run on this context");
    if (V <= 0) return SH_OK;
    std::lock_guard<std::mutex> lk(ps->mu);
    const int rc = patset_reserve(ps, st, V); if (rc) return rc;
    HIPCHK(shk_ps_insert_digests(st, d_digest, V, d_flags, d_n_missing, ps->k1, ps->k2, ps->slots, ps->cnt));
    ps->ub += V;
    return patset_mark(ps, st);
}

static int patset_stage(sh_ctx *c, const void *src, int64_t nbytes)
{
    PatSet *ps = c->patset;
    if (nbytes > ps->cap_stage) {
        HIPCHK(hipStreamSynchronize(c->stream));                        // (the insert of the call before reads the old buffer)
        hipFree(ps->d_stage); ps->d_stage = nullptr; ps->cap_stage = 0;
        if (hipMalloc((void **)&ps->d_stage, (size_t)nbytes) != hipSuccess) { (void)hipGetLastError(); return fail(SH_ENOMEM, "pattern set: no device memory for the rows"); }
        ps->cap_stage = nbytes;
    }
    // behind the insert of the call before, which reads the buffer; the caller's memory is pageable and free again when this returns
    HIPCHK(hipMemcpyAsync(ps->d_stage, src, (size_t)nbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SH_OK;
}

static void patset_free(sh_ctx *c)
{
    PatSet *ps = c->patset;
    if (!ps) return;
    (void)patset_drain(ps);
    hipFree(ps->k1); hipFree(ps->k2); hipFree(ps->cnt); hipFree(ps->d_stage);
    delete ps;
    c->patset = nullptr;
}

int sh_patset_begin(sh_ctx *c, int64_t initial_slots)
{
    if (!c) return fail(SH_EINVAL, "null ctx");
    if (c->patset) return fail(SH_EINVAL, "sh_patset_begin: the context has a pattern set already");
    if (initial_slots == 0) initial_slots = (int64_t)1 << 20;
    if (initial_slots < 1024 || (initial_slots & (initial_slots - 1)) || initial_slots > ((int64_t)1 << 40))
        return fail(SH_EINVAL, "sh_patset_begin: initial_slots must be 0 or a power of two >= 1024");
    HIPCHK(hipSetDevice(c->device));
    PatSet *ps = new PatSet();
    int rc = patset_table(initial_slots, c->stream, &ps->k1, &ps->k2);
    if (!rc && hipMalloc((void **)&ps->cnt, 16) != hipSuccess) { (void)hipGetLastError(); rc = fail(SH_ENOMEM, "pattern set: no device memory"); }
    if (!rc) {
        hipError_t e = hipMemsetAsync(ps->cnt, 0, 16, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);       // (the first insert may come on a lane's stream)
        if (e != hipSuccess) rc = fail(SH_EHIP, std::string("sh_patset_begin: ") + hipGetErrorString(e));
    }
    if (rc) { hipFree(ps->k1); hipFree(ps->k2); hipFree(ps->cnt); delete ps; return rc; }
    ps->slots = initial_slots;
    c->patset = ps;
    return SH_OK;
}

int sh_patset_add_rows_dev(sh_ctx *c, const void *d_bits, int64_t row_bytes, int64_t V)
{
    if (!c || !c->patset) return fail(SH_EINVAL, "sh_patset_add_rows: sh_patset_begin has not run on this context");
    if (V < 0 || row_bytes <= 0 || (V > 0 && !d_bits)) return fail(SH_EINVAL, "sh_patset_add_rows: bad argument");
    if (row_bytes * 8 < c->N) return fail(SH_ESHAPE, "row_bytes*8 < n_samples");
    HIPCHK(hipSetDevice(c->device));
    return patset_insert_rows(c, c->stream, (const uint8_t *)d_bits, row_bytes, V, nullptr);
}

int sh_patset_add_rows(sh_ctx *c, const uint8_t *bits, int64_t row_bytes, int64_t V)
{
    if (!c || !c->patset) return fail(SH_EINVAL, "sh_patset_add_rows: sh_patset_begin has not run on this context");
    if (V < 0 || row_bytes <= 0 || (V > 0 && !bits)) return fail(SH_EINVAL, "sh_patset_add_rows: bad argument");
    if (row_bytes * 8 < c->N) return fail(SH_ESHAPE, "row_bytes*8 < n_samples");
    if (V == 0) return SH_OK;
    HIPCHK(hipSetDevice(c->device));
    const int rc = patset_stage(c, bits, V * row_bytes); if (rc) return rc;
    return patset_insert_rows(c, c->stream, c->patset->d_stage, row_bytes, V, nullptr);
}

int sh_patset_add_keys(sh_ctx *c, const uint64_t *keys, int64_t n)
{
    if (!c || !c->patset) return fail(SH_EINVAL, "sh_patset_add_keys: sh_patset_begin has not run on this context");
    if (n < 0 || (n > 0 && !keys)) return fail(SH_EINVAL, "sh_patset_add_keys: bad argument");
    if (n == 0) return SH_OK;
    HIPCHK(hipSetDevice(c->device));
    int rc = patset_stage(c, keys, n * 16); if (rc) return rc;
    PatSet *ps = c->patset;
    std::lock_guard<std::mutex> lk(ps->mu);
    rc = patset_reserve(ps, c->stream, n); if (rc) return rc;
    HIPCHK(shk_ps_insert_keys(c->stream, (const uint64_t *)ps->d_stage, n, ps->k1, ps->k2, ps->slots, ps->cnt));
    ps->ub += n;
    return patset_mark(ps, c->stream);
}

int sh_patset_count(sh_ctx *c, int64_t *distinct, int64_t *slots, int64_t *growths)
{
    if (!c || !c->patset) return fail(SH_EINVAL, "sh_patset_count: sh_patset_begin has not run on this context");
    HIPCHK(hipSetDevice(c->device));
    int rc = lanes_wait(c); if (rc) return rc;                          // (a lane may be about to queue a block's insert)
    PatSet *ps = c->patset;
    std::lock_guard<std::mutex> lk(ps->mu);
    rc = patset_drain(ps); if (rc) return rc;
    unsigned long long h[2];
    rc = patset_read(ps, h); if (rc) return rc;
    if (distinct) *distinct = (int64_t)h[0];
    if (slots) *slots = ps->slots;
    if (growths) *growths = ps->growths;
    return SH_OK;
}

int sh_patset_end(sh_ctx *c)
{
    if (!c) return fail(SH_EINVAL, "null ctx");
    if (!c->patset) return SH_OK;
    HIPCHK(hipSetDevice(c->device));
    const int rc = lanes_wait(c);
    patset_free(c);
    return rc;
}

// the keys the device gives the same rows (patset_hash.h): host only, no context
int sh_patset_hash_rows(const uint8_t *bits, int64_t row_bytes, int64_t V, int n_samples, uint64_t *keys)
{
    if (V < 0 || row_bytes <= 0 || n_samples < 1 || (V > 0 && (!bits || !keys))) return fail(SH_EINVAL, "sh_patset_hash_rows: bad argument");
    if (row_bytes * 8 < n_samples) return fail(SH_ESHAPE, "row_bytes*8 < n_samples");
    const int nw = (n_samples + 63) >> 6;
    for (int64_t v = 0; v < V; ++v) {
        const uint8_t *row = bits + v * row_bytes;
        uint64_t a = 0, b = 0;
        for (int i = 0; i < nw; ++i) {
            const uint64_t w = ps_row_word(row, row_bytes, n_samples, i, false);
            a += ps_word0(w, (uint64_t)i); b += ps_word1(w, (uint64_t)i);
        }
        keys[2 * v] = ps_fin0(a); keys[2 * v + 1] = ps_fin1(b);
    }
    return SH_OK;
}
