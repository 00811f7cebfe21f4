// vcf_api.inc -- sh_vcf_* and sh_burden_fold (include/seerhip.h): the native VCF reader.  Host half: csrc/vcf_reader.cpp (container, lines, the
// nine fixed columns); device half: csrc/vcf_kernels.hip (the sample columns).  A call of sh_vcf_next works through its records in sub-batches:
// the sample columns of a sub-batch are copied as they stand into one of two pinned slabs (each record at a 16-byte aligned offset), go to the
// device with the records' offsets, and k_vcf_gt_pack writes their present / missing rows; while that runs, the host decodes and frames the
// next sub-batch into the other slab.  A record longer than a slab makes the slabs grow.  The rows of the whole call come back at its end.
// BCF takes the same pump: what a record puts into the slab is its GT vector alone (n_cols x L bytes, csrc/vcf_reader.cpp "BCF"), and the
// kernel is k_bcf_gt_pack.

struct sh_vcf {
    sh_ctx *ctx = nullptr;                                 // nullptr: the host tokeniser (shvcf::host_gt_pack) stands in for the kernel
    shvcf::Reader *rd = nullptr;
    int N = 0, row_words = 0, n_cols = 0;
    int32_t *d_col2idx = nullptr;
    size_t slab = 0;                                       // bytes per slab
    uint8_t *h_bytes[2] = {nullptr, nullptr}, *d_bytes[2] = {nullptr, nullptr};
    ShVcfRec *h_recs[2] = {nullptr, nullptr}, *d_recs[2] = {nullptr, nullptr};
    size_t cap_recs = 0;                                   // records per sub-batch
    hipEvent_t ev[2] = {nullptr, nullptr}; bool ev_used[2] = {false, false};
    uint32_t *d_present = nullptr, *d_missing = nullptr; int32_t *d_np = nullptr, *d_nm = nullptr; int64_t cap_rows = 0;
    bool have_pending = false; shvcf::Record pending;
    std::string names; std::vector<int64_t> name_off;
    int64_t stat_bytes = 0, stat_records = 0, stat_launches = 0;
    std::vector<uint8_t> host_bytes;                       // (host tokeniser) the sub-batch's sample columns
};

static void vcf_free_slabs(sh_vcf *r)
{
    for (int s = 0; s < 2; ++s) {
        if (r->h_bytes[s]) hipHostFree(r->h_bytes[s]);
        if (r->d_bytes[s]) hipFree(r->d_bytes[s]);
        r->h_bytes[s] = nullptr; r->d_bytes[s] = nullptr;
    }
}

static int vcf_alloc_slabs(sh_vcf *r, size_t bytes)
{
    vcf_free_slabs(r);
    bytes = (bytes + 4095) / 4096 * 4096;
    for (int s = 0; s < 2; ++s) {
        HIPCHK(hipHostMalloc((void **)&r->h_bytes[s], bytes, hipHostMallocDefault));
        HIPCHK(hipMalloc((void **)&r->d_bytes[s], bytes));
    }
    r->slab = bytes;
    return SH_OK;
}

static int vcf_ensure_rows(sh_vcf *r, int64_t rows)
{
    if (rows <= r->cap_rows) return SH_OK;
    hipFree(r->d_present); hipFree(r->d_missing); hipFree(r->d_np); hipFree(r->d_nm);
    r->d_present = r->d_missing = nullptr; r->d_np = r->d_nm = nullptr; r->cap_rows = 0;
    HIPCHK(dmalloc(&r->d_present, (size_t)rows * r->row_words)); HIPCHK(dmalloc(&r->d_missing, (size_t)rows * r->row_words));
    HIPCHK(dmalloc(&r->d_np, (size_t)rows)); HIPCHK(dmalloc(&r->d_nm, (size_t)rows));
    r->cap_rows = rows;
    return SH_OK;
}

void sh_vcf_close(sh_vcf *r)
{
    if (!r) return;
    if (r->ctx) {
        hipSetDevice(r->ctx->device);
        hipStreamSynchronize(r->ctx->stream);
        vcf_free_slabs(r);
        for (int s = 0; s < 2; ++s) {
            if (r->h_recs[s]) hipHostFree(r->h_recs[s]);
            if (r->d_recs[s]) hipFree(r->d_recs[s]);
            if (r->ev[s]) hipEventDestroy(r->ev[s]);
        }
        hipFree(r->d_col2idx); hipFree(r->d_present); hipFree(r->d_missing); hipFree(r->d_np); hipFree(r->d_nm);
    }
    if (r->rd) shvcf::close_file(r->rd);
    delete r;
}

static int vcf_open_device(sh_vcf *r)
{
    sh_ctx *c = r->ctx;
    HIPCHK(hipSetDevice(c->device));
    if (shk_vcf_lds_bytes(r->row_words) + 16512 > 65536) return fail(SH_ESHAPE, "too many samples for the VCF kernel's rows in LDS (at most 196 000)");
    r->cap_recs = 4096;
    for (int s = 0; s < 2; ++s) {
        HIPCHK(hipHostMalloc((void **)&r->h_recs[s], r->cap_recs * sizeof(ShVcfRec), hipHostMallocDefault));
        HIPCHK(dmalloc(&r->d_recs[s], r->cap_recs));
        HIPCHK(hipEventCreateWithFlags(&r->ev[s], hipEventDisableTiming));
    }
    HIPCHK(dmalloc(&r->d_col2idx, (size_t)std::max(1, r->n_cols)));
    HIPCHK(hipMemcpyAsync(r->d_col2idx, shvcf::col_to_sample(r->rd), sizeof(int32_t) * (size_t)r->n_cols, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return vcf_alloc_slabs(r, (size_t)32 << 20);
}

sh_vcf *sh_vcf_open(sh_ctx *ctx, const char *path, const char *const *sample_names, int n_samples)
{
    if (!path || !sample_names || n_samples < 1) { fail(SH_EINVAL, "bad argument"); return nullptr; }
    if (ctx && ctx->N != n_samples) { fail(SH_ESHAPE, "the context was created for another number of samples"); return nullptr; }
    std::string err;
    shvcf::Reader *rd = shvcf::open_file(path, sample_names, n_samples, err);
    if (!rd) { fail(SH_EINVAL, err); return nullptr; }
    sh_vcf *r = new sh_vcf();
    r->ctx = ctx; r->rd = rd; r->N = n_samples; r->row_words = (n_samples + 63) / 64 * 2; r->n_cols = shvcf::n_cols(rd);
    if (ctx && vcf_open_device(r) != SH_OK) { const std::string keep = g_err; sh_vcf_close(r); g_err = keep; return nullptr; }
    return r;
}

// one sub-batch on the device: bytes and record table up, the kernel, an event for the slab's next use
static int vcf_launch(sh_vcf *r, int slot, size_t used, int64_t nrec, int64_t row0)
{
    sh_ctx *c = r->ctx;
    if (used) HIPCHK(hipMemcpyAsync(r->d_bytes[slot], r->h_bytes[slot], used, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(r->d_recs[slot], r->h_recs[slot], sizeof(ShVcfRec) * (size_t)nrec, hipMemcpyHostToDevice, c->stream));
    HIPCHK((shvcf::format(r->rd) ? shk_bcf_gt_pack : shk_vcf_gt_pack)(c->stream, r->d_bytes[slot], r->d_recs[slot], nrec, r->d_col2idx, r->n_cols, r->row_words,
                           r->d_present + (size_t)row0 * r->row_words, r->d_missing + (size_t)row0 * r->row_words, r->d_np + row0, r->d_nm + row0));
    HIPCHK(hipEventRecord(r->ev[slot], c->stream));
    r->ev_used[slot] = true;
    r->stat_bytes += (int64_t)used; r->stat_launches += 1;
    return SH_OK;
}

int64_t sh_vcf_next(sh_vcf *r, int64_t max_records, int32_t *skip, int64_t *pos, int32_t *ref_len, int32_t *contig, uint8_t *present, uint8_t *missing,
                    int64_t row_bytes, int32_t *n_present, int32_t *n_missing)
{
    if (!r || !skip || !pos || !ref_len || !contig || !present || !missing || !n_present || !n_missing) { fail(SH_EINVAL, "null argument"); return -1; }
    if (row_bytes != (int64_t)r->row_words * 4) { fail(SH_ESHAPE, "row_bytes is not that of the reader's sample count"); return -1; }
    if (max_records < 1) return 0;
    sh_ctx *c = r->ctx;
    const bool bcf = shvcf::format(r->rd) != 0;
    if (c) {
        if (hipSetDevice(c->device) != hipSuccess) { fail(SH_EHIP, "hipSetDevice"); return -1; }
        if (vcf_ensure_rows(r, max_records) != SH_OK) return -1;
    }
    r->names.clear(); r->name_off.assign(1, 0);
    std::string err;
    int64_t done = 0;
    bool eof = false;
    int sb = 0;
    while (done < max_records && !eof) {
        const int slot = sb & 1;
        if (c && r->ev_used[slot]) { if (hipEventSynchronize(r->ev[slot]) != hipSuccess) { fail(SH_EHIP, "hipEventSynchronize"); return -1; } r->ev_used[slot] = false; }
        size_t used = 0;
        int64_t nrec = 0;
        if (!c) r->host_bytes.clear();
        std::vector<ShVcfRec> host_recs;
        while (done + nrec < max_records && (c == nullptr ? nrec < 4096 : nrec < (int64_t)r->cap_recs)) {
            if (!r->have_pending) {
                const int rc = shvcf::next(r->rd, r->pending, err);
                if (rc < 0) { fail(SH_EINVAL, err); return -1; }
                if (rc == 0) { eof = true; break; }
                r->have_pending = true;
            }
            const shvcf::Record &rec = r->pending;
            if (rec.samp_len >= ((size_t)1 << 31)) { fail(SH_EINVAL, "VCF: a record of 2 GB or more"); return -1; }
            const bool send = rec.skip == shvcf::KEPT && rec.gt >= 0;
            const size_t need = send ? (rec.samp_len + 15) / 16 * 16 : 0;
            if (c && used + need > r->slab) {
                if (nrec) break;                                          // the slab is full: this record opens the next sub-batch
                // a record longer than a slab: both slabs grow (the other one may still be in flight)
                if (hipStreamSynchronize(c->stream) != hipSuccess) { fail(SH_EHIP, "hipStreamSynchronize"); return -1; }
                r->ev_used[0] = r->ev_used[1] = false;
                if (vcf_alloc_slabs(r, need * 2) != SH_OK) return -1;
            }
            ShVcfRec d; d.off = used; d.len = send ? (uint32_t)rec.samp_len : 0u; d.gt = rec.skip != shvcf::KEPT ? -2 : rec.gt;
            if (bcf) d.len = send ? (uint32_t)rec.gt : 0u;                // (the GT vector's values per sample; its bytes are n_cols times that)
            if (c) {
                if (send) { memcpy(r->h_bytes[slot] + used, rec.samp, rec.samp_len); memset(r->h_bytes[slot] + used + rec.samp_len, 0, need - rec.samp_len); }
                r->h_recs[slot][nrec] = d;
            } else {
                if (send) r->host_bytes.insert(r->host_bytes.end(), rec.samp, rec.samp + rec.samp_len);
                d.off = r->host_bytes.size() - (send ? rec.samp_len : 0);
                host_recs.push_back(d);
            }
            used += c ? need : (send ? rec.samp_len : 0);
            const int64_t i = done + nrec;
            skip[i] = rec.skip; pos[i] = rec.pos; ref_len[i] = rec.ref_len; contig[i] = rec.contig;
            r->names.append(rec.name, rec.name_len); r->name_off.push_back((int64_t)r->names.size());
            r->have_pending = false;
            ++nrec;
        }
        if (nrec == 0) break;
        if (c) {
            if (vcf_launch(r, slot, used, nrec, done) != SH_OK) return -1;
        } else {
            const int32_t *c2i = shvcf::col_to_sample(r->rd);
            memset(present + (size_t)done * row_bytes, 0, (size_t)nrec * row_bytes); memset(missing + (size_t)done * row_bytes, 0, (size_t)nrec * row_bytes);
            const std::function<void(int64_t)> fn = [&](int64_t k) {
                const ShVcfRec &d = host_recs[(size_t)k];
                uint32_t *const P = (uint32_t *)(present + (size_t)(done + k) * row_bytes), *const M = (uint32_t *)(missing + (size_t)(done + k) * row_bytes);
                if (bcf) shvcf::host_bcf_pack(r->host_bytes.data() + d.off, d.len, d.gt, c2i, r->n_cols, P, M, r->row_words, n_present + done + k, n_missing + done + k);
                else shvcf::host_gt_pack(r->host_bytes.data() + d.off, d.len, d.gt, c2i, r->n_cols, P, M, r->row_words, n_present + done + k, n_missing + done + k);
            };
            shost::pool().run(nrec, 1, fn, shost::ST_READER_PARSE);
            r->stat_bytes += (int64_t)used;
        }
        done += nrec; ++sb;
    }
    r->stat_records += done;
    if (c && done) {
        hipError_t e = hipMemcpyAsync(present, r->d_present, (size_t)done * row_bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(missing, r->d_missing, (size_t)done * row_bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(n_present, r->d_np, sizeof(int32_t) * (size_t)done, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(n_missing, r->d_nm, sizeof(int32_t) * (size_t)done, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { fail(SH_EHIP, std::string("sh_vcf_next: ") + hipGetErrorString(e)); return -1; }
        r->ev_used[0] = r->ev_used[1] = false;
    }
    return done;
}

int64_t sh_vcf_names(sh_vcf *r, const char **blob, const int64_t **name_off)
{
    if (!r || !blob || !name_off) return fail(SH_EINVAL, "null argument");
    *blob = r->names.data(); *name_off = r->name_off.data();
    return (int64_t)r->names.size();
}

int sh_vcf_info(sh_vcf *r, int *mode, int *n_cols, int *n_contigs)
{
    if (!r) return fail(SH_EINVAL, "null reader");
    if (mode) *mode = shvcf::mode(r->rd);
    if (n_cols) *n_cols = r->n_cols;
    if (n_contigs) *n_contigs = shvcf::n_contigs(r->rd);
    return SH_OK;
}

int sh_vcf_format(sh_vcf *r) { return r ? shvcf::format(r->rd) : fail(SH_EINVAL, "null reader"); }

const char *sh_vcf_contig(sh_vcf *r, int id) { return r ? shvcf::contig_name(r->rd, id) : ""; }

int sh_vcf_stats(sh_vcf *r, int64_t *sample_bytes, int64_t *records, int64_t *launches)
{
    if (!r) return fail(SH_EINVAL, "null reader");
    if (sample_bytes) *sample_bytes = r->stat_bytes;
    if (records) *records = r->stat_records;
    if (launches) *launches = r->stat_launches;
    return SH_OK;
}

int sh_burden_fold(sh_ctx *c, const uint8_t *present, const uint8_t *missing, int64_t row_bytes, int64_t n_records, const int64_t *csr_off, const int32_t *csr_idx,
                   int64_t n_variants, uint8_t *out_present, uint8_t *out_missing, int32_t *n_present, int32_t *n_missing)
{
    if (!c) return fail(SH_EINVAL, "null ctx");
    if (!csr_off || !out_present || !out_missing || !n_present || !n_missing || (n_records > 0 && (!present || !missing))) return fail(SH_EINVAL, "null argument");
    if (row_bytes % 4 || row_bytes * 8 < c->N) return fail(SH_ESHAPE, "row_bytes does not fit n_samples");
    if (n_variants <= 0) return SH_OK;
    if (csr_off[0] != 0) return fail(SH_EINVAL, "csr_off[0] must be 0");
    for (int64_t v = 0; v < n_variants; ++v) if (csr_off[v + 1] < csr_off[v]) return fail(SH_EINVAL, "csr_off must not decrease");
    const int64_t nnz = csr_off[n_variants];
    if (nnz > 0 && !csr_idx) return fail(SH_EINVAL, "null argument");
    for (int64_t k = 0; k < nnz; ++k) if (csr_idx[k] < 0 || csr_idx[k] >= n_records) return fail(SH_EINVAL, "a record index outside the batch");
    HIPCHK(hipSetDevice(c->device));
    const int row_words = (int)(row_bytes / 4);
    uint32_t *d_p = nullptr, *d_m = nullptr, *d_op = nullptr, *d_om = nullptr; int64_t *d_off = nullptr; int32_t *d_idx = nullptr, *d_np = nullptr, *d_nm = nullptr;
    int rc = SH_OK;
    auto chk = [&](hipError_t e, const char *what) { if (e != hipSuccess && rc == SH_OK) rc = fail(SH_EHIP, std::string(what) + ": " + hipGetErrorString(e)); return e == hipSuccess; };
    const size_t in_words = (size_t)std::max<int64_t>(1, n_records) * row_words, out_words = (size_t)n_variants * row_words;
    if (chk(dmalloc(&d_p, in_words), "hipMalloc") && chk(dmalloc(&d_m, in_words), "hipMalloc") && chk(dmalloc(&d_op, out_words), "hipMalloc")
        && chk(dmalloc(&d_om, out_words), "hipMalloc") && chk(dmalloc(&d_off, (size_t)n_variants + 1), "hipMalloc") && chk(dmalloc(&d_idx, (size_t)std::max<int64_t>(1, nnz)), "hipMalloc")
        && chk(dmalloc(&d_np, (size_t)n_variants), "hipMalloc") && chk(dmalloc(&d_nm, (size_t)n_variants), "hipMalloc")) {
        if (n_records > 0) {
            chk(hipMemcpyAsync(d_p, present, (size_t)n_records * row_bytes, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
            chk(hipMemcpyAsync(d_m, missing, (size_t)n_records * row_bytes, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
        }
        chk(hipMemcpyAsync(d_off, csr_off, sizeof(int64_t) * ((size_t)n_variants + 1), hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
        if (nnz > 0) chk(hipMemcpyAsync(d_idx, csr_idx, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
        if (rc == SH_OK) chk(shk_burden_fold(c->stream, d_p, d_m, row_words, n_records, d_off, d_idx, n_variants, d_op, d_om, d_np, d_nm), "k_burden_fold");
        if (rc == SH_OK) {
            chk(hipMemcpyAsync(out_present, d_op, (size_t)n_variants * row_bytes, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
            chk(hipMemcpyAsync(out_missing, d_om, (size_t)n_variants * row_bytes, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
            chk(hipMemcpyAsync(n_present, d_np, sizeof(int32_t) * (size_t)n_variants, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
            chk(hipMemcpyAsync(n_missing, d_nm, sizeof(int32_t) * (size_t)n_variants, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
        }
        chk(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    }
    hipFree(d_p); hipFree(d_m); hipFree(d_op); hipFree(d_om); hipFree(d_off); hipFree(d_idx); hipFree(d_np); hipFree(d_nm);
    return rc;
}
