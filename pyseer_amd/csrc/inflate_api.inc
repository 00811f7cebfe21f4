// inflate_api.inc -- the device inflate of the k-mer reader's device route (include/seerhip.h: SEERHIP_ROUTE kmer_inflate=1, sh_inflate_host,
// sh_inflate_members_dev, sh_reader_dev_inflate_stats).  The reader (csrc/reader.cpp) frames the BGZF members of a slab as it always did and
// hands them to the hook below instead of its decoding threads, once per slab, on its decoding thread:
//   the members' deflate bodies go into one pinned staging buffer, one after the other, and up -- about a fifth of the text;
//   k_bgzf_inflate (inflate_kernels.hip) writes the text into the device copy of the slab, in the slab's own layout;
//   the text comes back by DMA into the pinned slab at buf + pad, for the reader's CRC-32, newline index and names;
//   one wait for the stream -- the hook's own, neither the context's nor the one slab_in and k_kmer_pack use, which belongs to the
//   consuming thread -- and the statuses are read.
// The device copy is left in KmerDev::inflated; slab_in binds it to the slab and uploads only the carried tail in front of the pad and the
// members the reader decoded again (kmer_api.inc).  Without a context the hook runs shi_inflate (inflate_dev.h), the kernel's text built for
// the host, straight into the slab.

static bool kmer_inflate_ensure(KmerDev *k, size_t comp_bytes, int64_t n, std::string &err)
{
    if (!k->istream) {
        if (!kmer_hip(hipStreamCreateWithFlags(&k->istream, hipStreamNonBlocking), "hipStreamCreate (inflate)", err)) return false;
        if (!kmer_hip(hipEventCreate(&k->i0), "hipEventCreate", err) || !kmer_hip(hipEventCreate(&k->i1), "hipEventCreate", err)) return false;
    }
    // (the stream is idle between two calls of the hook: nothing reads what is freed here)
    if (comp_bytes > k->cap_comp) {
        const size_t cap = std::max<size_t>(comp_bytes * 3 / 2, (size_t)1 << 20);
        if (k->h_comp) hipHostFree(k->h_comp);
        hipFree(k->d_comp);
        k->h_comp = k->d_comp = nullptr; k->cap_comp = 0;
        if (!kmer_hip(hipHostMalloc((void **)&k->h_comp, cap, hipHostMallocDefault), "hipHostMalloc (compressed members)", err)) return false;
        if (!kmer_hip(hipMalloc((void **)&k->d_comp, cap), "hipMalloc (compressed members)", err)) return false;
        k->cap_comp = cap;
    }
    if (n > k->cap_mem) {
        const int64_t cap = std::max<int64_t>(n * 2, 1024);
        if (k->h_mem) hipHostFree(k->h_mem);
        hipFree(k->d_mem);
        k->h_mem = k->d_mem = nullptr; k->cap_mem = 0;
        if (!kmer_hip(hipHostMalloc((void **)&k->h_mem, (size_t)cap * (sizeof(ShInfMember) + 8), hipHostMallocDefault), "hipHostMalloc (member table)", err)) return false;
        if (!kmer_hip(hipMalloc((void **)&k->d_mem, (size_t)cap * (sizeof(ShInfMember) + 8)), "hipMalloc (member table)", err)) return false;
        k->cap_mem = cap;
    }
    return true;
}

static bool kmer_inflate(void *self, char *buf, size_t pad, ShReaderMember *mem, int64_t n, std::string &err)
{
    KmerDev *k = (KmerDev *)self;
    if (!k->ctx) {
        const std::function<void(int64_t)> fn = [&](int64_t i) {
            static thread_local ShInfTables tables;
            ShReaderMember &m = mem[i];
            m.status = shi_inflate(m.cdata, m.clen, (uint8_t *)buf + pad + m.off, m.isize, &tables, &m.produced, ShInfOne());
        };
        shost::pool().run(n, 4, fn, shost::ST_READER_DECODE);
        k->members_dev += n;
        std::lock_guard<std::mutex> lk(k->mu);
        k->inflated[buf] = KmerDev::Copy();
        return true;
    }
    if (!kmer_hip(hipSetDevice(k->device), "hipSetDevice", err)) return false;
    KmerDev::Copy c;
    if (!kmer_copy_take(k, buf, c, err)) return false;
    const auto keep = [&](bool ok) { std::lock_guard<std::mutex> lk(k->mu); k->inflated[buf] = c; return ok; };      // (the copy is never lost)
    size_t comp_bytes = 0, text_bytes = 0;
    for (int64_t i = 0; i < n; ++i) { comp_bytes += mem[i].clen; text_bytes = std::max(text_bytes, mem[i].off + mem[i].isize); }
    if (pad + text_bytes > k->buf_bytes.load()) { err = "device k-mer reader: a slab's members decode to more than the slab holds"; return keep(false); }
    if (n > 0) {
        if (!kmer_inflate_ensure(k, comp_bytes + 8, n, err)) return keep(false);
        ShInfMember *hm = (ShInfMember *)k->h_mem;
        size_t at = 0;
        for (int64_t i = 0; i < n; ++i) {
            memcpy(k->h_comp + at, mem[i].cdata, mem[i].clen);
            hm[i].coff = at; hm[i].ooff = pad + mem[i].off; hm[i].clen = mem[i].clen; hm[i].isize = mem[i].isize;
            at += mem[i].clen;
        }
        int32_t *h_st = (int32_t *)(k->h_mem + (size_t)n * sizeof(ShInfMember)), *d_st = (int32_t *)(k->d_mem + (size_t)n * sizeof(ShInfMember));
        const bool ok =
            kmer_hip(hipMemcpyAsync(k->d_comp, k->h_comp, comp_bytes, hipMemcpyHostToDevice, k->istream), "hipMemcpyAsync (compressed members)", err) &&
            kmer_hip(hipMemcpyAsync(k->d_mem, k->h_mem, (size_t)n * sizeof(ShInfMember), hipMemcpyHostToDevice, k->istream), "hipMemcpyAsync (member table)", err) &&
            kmer_hip(hipEventRecord(k->i0, k->istream), "hipEventRecord", err) &&
            kmer_hip(shk_bgzf_inflate(k->istream, k->d_comp, (const ShInfMember *)k->d_mem, n, c.d, d_st, (uint32_t *)(d_st + n)), "k_bgzf_inflate", err) &&
            kmer_hip(hipEventRecord(k->i1, k->istream), "hipEventRecord", err) &&
            (text_bytes == 0 || kmer_hip(hipMemcpyAsync(buf + pad, c.d + pad, text_bytes, hipMemcpyDeviceToHost, k->istream), "hipMemcpyAsync (text)", err)) &&
            kmer_hip(hipMemcpyAsync(h_st, d_st, (size_t)n * 8, hipMemcpyDeviceToHost, k->istream), "hipMemcpyAsync (statuses)", err) &&
            kmer_hip(hipStreamSynchronize(k->istream), "hipStreamSynchronize (inflate)", err);
        if (!ok) return keep(false);
        for (int64_t i = 0; i < n; ++i) { mem[i].status = h_st[i]; mem[i].produced = (uint32_t)h_st[n + i]; }
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, k->i0, k->i1) == hipSuccess) k->infl_ms.store(k->infl_ms.load() + (double)ms);
        k->members_dev += n; k->infl_up += (int64_t)(comp_bytes + (size_t)n * sizeof(ShInfMember)); k->infl_down += (int64_t)(text_bytes + (size_t)n * 8);
    }
    return keep(true);
}

int sh_inflate_host(const uint8_t *cdata, int64_t clen, uint8_t *out, int64_t isize, int64_t *produced)
{
    if (clen < 0 || isize < 0 || clen > 0x7fffffff || isize > 0x7fffffff || (clen && !cdata) || (isize && !out)) return fail(SH_EINVAL, "bad argument");
    ShInfTables *t = new ShInfTables;
    uint32_t n = 0;
    const int st = shi_inflate(cdata, (uint32_t)clen, out, (uint32_t)isize, t, &n, ShInfOne());
    delete t;
    if (produced) *produced = (int64_t)n;
    return st;
}

int sh_inflate_members_dev(sh_ctx *ctx, const uint8_t *comp, int64_t comp_bytes, const int64_t *coff, const int32_t *clen, const int32_t *isize,
                           const int64_t *ooff, int64_t n, uint8_t *out, int64_t out_bytes, int32_t *status, int32_t *produced, double *kernel_ms)
{
    if (!ctx || !comp || !coff || !clen || !isize || !ooff || !out || !status || !produced || n < 1 || comp_bytes < 1 || out_bytes < 1) return fail(SH_EINVAL, "bad argument");
    std::vector<ShInfMember> hm((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        // every range the kernel may touch lies in the buffers it gets
        if (coff[i] < 0 || clen[i] < 0 || clen[i] > (1 << 20) || coff[i] > comp_bytes - clen[i]) return fail(SH_EINVAL, "a member's compressed bytes lie outside the buffer (or are more than 1 MB)");
        if (ooff[i] < 0 || isize[i] < 0 || isize[i] > (int32_t)SHI_MEMBER_MAX || ooff[i] > out_bytes - isize[i]) return fail(SH_EINVAL, "a member's text lies outside the buffer (or is more than 64 KB)");
        hm[(size_t)i] = ShInfMember{(uint64_t)coff[i], (uint64_t)ooff[i], (uint32_t)clen[i], (uint32_t)isize[i]};
    }
    HIPCHK(hipSetDevice(ctx->device));
    uint8_t *d_comp = nullptr, *d_out = nullptr; ShInfMember *d_mem = nullptr; int32_t *d_st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const auto run = [&]() -> hipError_t {
        hipError_t e;
        // (eight bytes of slack: the bit buffer is refilled eight bytes at a time, though never past a member's end)
        if ((e = hipMalloc((void **)&d_comp, (size_t)comp_bytes + 8)) != hipSuccess || (e = hipMalloc((void **)&d_out, (size_t)out_bytes)) != hipSuccess) return e;
        if ((e = dmalloc(&d_mem, (size_t)n)) != hipSuccess || (e = dmalloc(&d_st, (size_t)n * 2)) != hipSuccess) return e;
        if ((e = hipEventCreate(&e0)) != hipSuccess || (e = hipEventCreate(&e1)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(d_comp, comp, (size_t)comp_bytes, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(d_out, out, (size_t)out_bytes, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(d_mem, hm.data(), (size_t)n * sizeof(ShInfMember), hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) return e;
        if ((e = hipEventRecord(e0, ctx->stream)) != hipSuccess) return e;
        if ((e = shk_bgzf_inflate(ctx->stream, d_comp, d_mem, n, d_out, d_st, (uint32_t *)(d_st + n))) != hipSuccess) return e;
        if ((e = hipEventRecord(e1, ctx->stream)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(out, d_out, (size_t)out_bytes, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(status, d_st, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(produced, d_st + n, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return e;
        float ms = 0.0f;
        if (kernel_ms) { if ((e = hipEventElapsedTime(&ms, e0, e1)) != hipSuccess) return e; *kernel_ms = (double)ms; }
        return hipSuccess;
    };
    const hipError_t e = run();
    if (e != hipSuccess) hipStreamSynchronize(ctx->stream);
    hipFree(d_comp); hipFree(d_out); hipFree(d_mem); hipFree(d_st);
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    if (e != hipSuccess) return fail(SH_EHIP, std::string("sh_inflate_members_dev: ") + hipGetErrorString(e));
    return SH_OK;
}

int sh_reader_dev_inflate_stats(sh_reader *r, int64_t *members_dev, int64_t *members_host, int64_t *bytes_up, int64_t *bytes_down, double *kernel_ms)
{
    KmerDev *k = (KmerDev *)sh_reader_hooks_self(r);
    if (!k) return fail(SH_EINVAL, "not a reader opened by sh_reader_open_dev");
    if (members_dev) *members_dev = k->members_dev.load();
    if (members_host) *members_host = k->members_host.load();
    if (bytes_up) *bytes_up = k->infl_up;
    if (bytes_down) *bytes_down = k->infl_down;
    if (kernel_ms) *kernel_ms = k->infl_ms.load();
    return SH_OK;
}
