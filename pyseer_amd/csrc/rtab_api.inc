// rtab_api.inc -- sh_rtab_* (include/seerhip.h): the native Rtab reader.  Host half: csrc/rtab_reader.cpp (framing, trailing strip, the name);
// device half: csrc/rtab_kernels.hip (the calls).  The scheme is that of vcf_api.inc, kept apart from it so that sh_vcf_next stays as it is: a
// call of sh_rtab_next works through its lines in sub-batches; the call text of a sub-batch is copied as it stands into one of two pinned slabs
// (each line at a 16-byte aligned offset, padded with zeros), goes to the device with the lines' offsets, and k_rtab_pack writes status, rows
// and counts; while that runs, the host frames the next sub-batch into the other slab.  A line longer than a slab makes the slabs grow.  The
// rows of the whole call come back at its end.  A malformed line is a status, not an error.

struct sh_rtab {
    sh_ctx *ctx = nullptr;                                 // nullptr: the host tokeniser (shrtab::host_rtab_pack) stands in for the kernel
    shrtab::Reader *rd = nullptr;
    int N = 0, row_words = 0, n_cols = 0, wg = 0;
    int32_t *d_col2idx = nullptr;
    size_t slab = 0;                                       // bytes per slab
    uint8_t *h_bytes[2] = {nullptr, nullptr}, *d_bytes[2] = {nullptr, nullptr};
    ShRtabRec *h_recs[2] = {nullptr, nullptr}, *d_recs[2] = {nullptr, nullptr};
    size_t cap_recs = 0;                                   // lines per sub-batch
    hipEvent_t ev[2] = {nullptr, nullptr}; bool ev_used[2] = {false, false};
    uint32_t *d_present = nullptr, *d_missing = nullptr; int32_t *d_np = nullptr, *d_nm = nullptr, *d_status = nullptr; int64_t cap_rows = 0;
    bool have_pending = false; shrtab::Line pending;
    std::string names; std::vector<int64_t> name_off;
    int64_t stat_bytes = 0, stat_rows = 0, stat_launches = 0;
    std::vector<shrtab::Line> host_lines;                  // (host tokeniser) the sub-batch's lines, in the file's mapping
};

static void rtab_free_slabs(sh_rtab *r)
{
    for (int s = 0; s < 2; ++s) {
        if (r->h_bytes[s]) hipHostFree(r->h_bytes[s]);
        if (r->d_bytes[s]) hipFree(r->d_bytes[s]);
        r->h_bytes[s] = nullptr; r->d_bytes[s] = nullptr;
    }
}

static int rtab_alloc_slabs(sh_rtab *r, size_t bytes)
{
    rtab_free_slabs(r);
    bytes = (bytes + 4095) / 4096 * 4096;
    for (int s = 0; s < 2; ++s) {
        HIPCHK(hipHostMalloc((void **)&r->h_bytes[s], bytes, hipHostMallocDefault));
        HIPCHK(hipMalloc((void **)&r->d_bytes[s], bytes));
    }
    r->slab = bytes;
    return SH_OK;
}

static int rtab_ensure_rows(sh_rtab *r, int64_t rows)
{
    if (rows <= r->cap_rows) return SH_OK;
    hipFree(r->d_present); hipFree(r->d_missing); hipFree(r->d_np); hipFree(r->d_nm); hipFree(r->d_status);
    r->d_present = r->d_missing = nullptr; r->d_np = r->d_nm = r->d_status = nullptr; r->cap_rows = 0;
    HIPCHK(dmalloc(&r->d_present, (size_t)rows * r->row_words)); HIPCHK(dmalloc(&r->d_missing, (size_t)rows * r->row_words));
    HIPCHK(dmalloc(&r->d_np, (size_t)rows)); HIPCHK(dmalloc(&r->d_nm, (size_t)rows)); HIPCHK(dmalloc(&r->d_status, (size_t)rows));
    r->cap_rows = rows;
    return SH_OK;
}

void sh_rtab_close(sh_rtab *r)
{
    if (!r) return;
    if (r->ctx) {
        hipSetDevice(r->ctx->device);
        hipStreamSynchronize(r->ctx->stream);
        rtab_free_slabs(r);
        for (int s = 0; s < 2; ++s) {
            if (r->h_recs[s]) hipHostFree(r->h_recs[s]);
            if (r->d_recs[s]) hipFree(r->d_recs[s]);
            if (r->ev[s]) hipEventDestroy(r->ev[s]);
        }
        hipFree(r->d_col2idx); hipFree(r->d_present); hipFree(r->d_missing); hipFree(r->d_np); hipFree(r->d_nm); hipFree(r->d_status);
    }
    if (r->rd) shrtab::close_file(r->rd);
    delete r;
}

static int rtab_open_device(sh_rtab *r, size_t slab_bytes)
{
    sh_ctx *c = r->ctx;
    HIPCHK(hipSetDevice(c->device));
    if (shk_rtab_lds_bytes(r->row_words) + 128 > 65536) return fail(SH_ESHAPE, "too many samples for the Rtab kernel's rows in LDS (at most 261 000)");
    r->cap_recs = 8192;
    for (int s = 0; s < 2; ++s) {
        HIPCHK(hipHostMalloc((void **)&r->h_recs[s], r->cap_recs * sizeof(ShRtabRec), hipHostMallocDefault));
        HIPCHK(dmalloc(&r->d_recs[s], r->cap_recs));
        HIPCHK(hipEventCreateWithFlags(&r->ev[s], hipEventDisableTiming));
    }
    HIPCHK(dmalloc(&r->d_col2idx, (size_t)std::max(1, r->n_cols)));
    if (r->n_cols) HIPCHK(hipMemcpyAsync(r->d_col2idx, shrtab::col_to_sample(r->rd), sizeof(int32_t) * (size_t)r->n_cols, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return rtab_alloc_slabs(r, slab_bytes);
}

sh_rtab *sh_rtab_open(sh_ctx *ctx, const char *path, const char *const *sample_names, int n_samples, const char *const *columns, int n_columns)
{
    if (!path || !sample_names || n_samples < 1 || n_columns < 0 || (n_columns > 0 && !columns)) { fail(SH_EINVAL, "bad argument"); return nullptr; }
    if (ctx && ctx->N != n_samples) { fail(SH_ESHAPE, "the context was created for another number of samples"); return nullptr; }
    int wg = 0;
    size_t slab_bytes = (size_t)32 << 20;
    if (const char *v = sh_route("rtab_wg")) {
        wg = atoi(v);
        if (wg != 64 && wg != 256) { fail(SH_EINVAL, "SEERHIP_ROUTE: rtab_wg is 64 or 256"); return nullptr; }
    }
    if (const char *v = sh_route("rtab_slab")) slab_bytes = (size_t)std::max(16, atoi(v));
    std::string err;
    bool dup = false;                                      // (err then begins "Rtab: duplicate sample column": what the callers look for)
    shrtab::Reader *rd = shrtab::open_file(path, sample_names, n_samples, columns, n_columns, err, dup);
    if (!rd) { fail(SH_EINVAL, err); return nullptr; }
    sh_rtab *r = new sh_rtab();
    r->ctx = ctx; r->rd = rd; r->N = n_samples; r->row_words = (n_samples + 63) / 64 * 2; r->n_cols = shrtab::n_cols(rd); r->wg = wg;
    if (ctx && rtab_open_device(r, slab_bytes) != SH_OK) { const std::string keep = g_err; sh_rtab_close(r); g_err = keep; return nullptr; }
    return r;
}

// one sub-batch on the device: bytes and line table up, the kernel, an event for the slab's next use
static int rtab_launch(sh_rtab *r, int slot, size_t used, int64_t nrec, int64_t row0)
{
    sh_ctx *c = r->ctx;
    if (used) HIPCHK(hipMemcpyAsync(r->d_bytes[slot], r->h_bytes[slot], used, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(r->d_recs[slot], r->h_recs[slot], sizeof(ShRtabRec) * (size_t)nrec, hipMemcpyHostToDevice, c->stream));
    HIPCHK(shk_rtab_pack(c->stream, r->wg, r->d_bytes[slot], r->d_recs[slot], nrec, r->d_col2idx, r->n_cols, r->row_words,
                         r->d_present + (size_t)row0 * r->row_words, r->d_missing + (size_t)row0 * r->row_words, r->d_np + row0, r->d_nm + row0, r->d_status + row0));
    HIPCHK(hipEventRecord(r->ev[slot], c->stream));
    r->ev_used[slot] = true;
    r->stat_bytes += (int64_t)used; r->stat_launches += 1;
    return SH_OK;
}

int64_t sh_rtab_next(sh_rtab *r, int64_t max_rows, int32_t *status, uint8_t *present, uint8_t *missing, int64_t row_bytes, int32_t *n_present, int32_t *n_missing)
{
    if (!r || !status || !present || !missing || !n_present || !n_missing) { fail(SH_EINVAL, "null argument"); return -1; }
    if (row_bytes != (int64_t)r->row_words * 4) { fail(SH_ESHAPE, "row_bytes is not that of the reader's sample count"); return -1; }
    if (max_rows < 1) return 0;
    sh_ctx *c = r->ctx;
    if (c) {
        if (hipSetDevice(c->device) != hipSuccess) { fail(SH_EHIP, "hipSetDevice"); return -1; }
        if (rtab_ensure_rows(r, max_rows) != SH_OK) return -1;
    }
    r->names.clear(); r->name_off.assign(1, 0);
    int64_t done = 0;
    bool eof = false;
    int sb = 0;
    while (done < max_rows && !eof) {
        const int slot = sb & 1;
        if (c && r->ev_used[slot]) { if (hipEventSynchronize(r->ev[slot]) != hipSuccess) { fail(SH_EHIP, "hipEventSynchronize"); return -1; } r->ev_used[slot] = false; }
        size_t used = 0;
        int64_t nrec = 0;
        r->host_lines.clear();
        while (done + nrec < max_rows && (c == nullptr ? nrec < 4096 : nrec < (int64_t)r->cap_recs)) {
            if (!r->have_pending) {
                if (shrtab::next(r->rd, r->pending) == 0) { eof = true; break; }
                r->have_pending = true;
            }
            const shrtab::Line &ln = r->pending;
            if (ln.calls_len >= ((size_t)1 << 31)) { fail(SH_EINVAL, "Rtab: a line of 2 GB or more"); return -1; }
            const size_t need = (ln.calls_len + 15) / 16 * 16;
            if (c && used + need > r->slab) {
                if (nrec) break;                                          // the slab is full: this line opens the next sub-batch
                // a line longer than a slab: both slabs grow (the other one may still be in flight)
                if (hipStreamSynchronize(c->stream) != hipSuccess) { fail(SH_EHIP, "hipStreamSynchronize"); return -1; }
                r->ev_used[0] = r->ev_used[1] = false;
                if (rtab_alloc_slabs(r, need * 2) != SH_OK) return -1;
            }
            if (c) {
                ShRtabRec d; d.off = used; d.len = (uint32_t)ln.calls_len; d.has_calls = ln.has_calls ? 1 : 0;
                if (need) { memcpy(r->h_bytes[slot] + used, ln.calls, ln.calls_len); memset(r->h_bytes[slot] + used + ln.calls_len, 0, need - ln.calls_len); }
                r->h_recs[slot][nrec] = d;
                used += need;
            } else {
                r->host_lines.push_back(ln);
                used += ln.calls_len;
            }
            r->names.append(ln.name, ln.name_len); r->name_off.push_back((int64_t)r->names.size());
            r->have_pending = false;
            ++nrec;
        }
        if (nrec == 0) break;
        if (c) {
            if (rtab_launch(r, slot, used, nrec, done) != SH_OK) return -1;
        } else {
            const int32_t *c2i = shrtab::col_to_sample(r->rd);
            memset(present + (size_t)done * row_bytes, 0, (size_t)nrec * row_bytes); memset(missing + (size_t)done * row_bytes, 0, (size_t)nrec * row_bytes);
            const std::function<void(int64_t)> fn = [&](int64_t k) {
                const shrtab::Line &ln = r->host_lines[(size_t)k];
                status[done + k] = shrtab::host_rtab_pack(ln.calls, ln.calls_len, ln.has_calls, c2i, r->n_cols, (uint32_t *)(present + (size_t)(done + k) * row_bytes),
                                                          (uint32_t *)(missing + (size_t)(done + k) * row_bytes), r->row_words, n_present + done + k, n_missing + done + k);
            };
            shost::pool().run(nrec, 1, fn, shost::ST_READER_PARSE);
            r->stat_bytes += (int64_t)used;
        }
        done += nrec; ++sb;
    }
    r->stat_rows += done;
    if (c && done) {
        hipError_t e = hipMemcpyAsync(present, r->d_present, (size_t)done * row_bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(missing, r->d_missing, (size_t)done * row_bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(n_present, r->d_np, sizeof(int32_t) * (size_t)done, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(n_missing, r->d_nm, sizeof(int32_t) * (size_t)done, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(status, r->d_status, sizeof(int32_t) * (size_t)done, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { fail(SH_EHIP, std::string("sh_rtab_next: ") + hipGetErrorString(e)); return -1; }
        r->ev_used[0] = r->ev_used[1] = false;
    }
    return done;
}

int64_t sh_rtab_names(sh_rtab *r, const char **blob, const int64_t **name_off)
{
    if (!r || !blob || !name_off) return fail(SH_EINVAL, "null argument");
    *blob = r->names.data(); *name_off = r->name_off.data();
    return (int64_t)r->names.size();
}

int sh_rtab_stats(sh_rtab *r, int64_t *call_bytes, int64_t *rows, int64_t *launches)
{
    if (!r) return fail(SH_EINVAL, "null reader");
    if (call_bytes) *call_bytes = r->stat_bytes;
    if (rows) *rows = r->stat_rows;
    if (launches) *launches = r->stat_launches;
    return SH_OK;
}

int sh_rtab_partition(sh_rtab *r, int *lane_bytes, int *wave_bytes, int *step_bytes)
{
    if (!r) return fail(SH_EINVAL, "null reader");
    if (lane_bytes) *lane_bytes = RTAB_LANE_BYTES;
    if (wave_bytes) *wave_bytes = RTAB_WAVE_BYTES;
    if (step_bytes) *step_bytes = (r->wg ? r->wg : shk_rtab_default_wg()) * RTAB_LANE_BYTES;
    return SH_OK;
}
