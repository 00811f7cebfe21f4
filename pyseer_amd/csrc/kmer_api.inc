// kmer_api.inc -- sh_reader_open_dev (include/seerhip.h): the device half of the k-mer reader's device route.  The reader itself
// (csrc/reader.cpp) knows nothing of HIP; it is opened with the hooks below (csrc/reader_dev.h):
//   alloc / release   its slab buffers are pinned memory, so the decoders write their text where the copy engine reads it;
//   slab_in           a slab has arrived (CRC checked): its text, pad included, goes to the device once, into a device buffer of the same
//                     layout, by hipMemcpyAsync on the reader's own stream; an event says when the pinned buffer may be written again;
//   slab_out          the reader lets the slab go: the event is waited for and the device buffer is kept for the next slab (the stream
//                     orders the next upload behind the kernels that read the old text);
//   pack              the framed lines of one sh_reader_next: one line table up, one k_kmer_pack, rows and counts back into pinned memory,
//                     one wait for the stream -- the reader's, never the context's -- and the rows copied to where the caller wants them.
// A line that lies in no slab (longer than the pad and straddling two slabs; every line under SEERHIP_ROUTE reader=zlib) and every line of
// a reader without a context goes through host_kmer_pack (csrc/kmer_kernels.h), the kernel's rule in plain C++.

struct KmerDev {
    sh_ctx *ctx = nullptr; int device = 0, N = 0, row_words = 0;
    hipStream_t stream = nullptr;
    // the sample table: the names as one blob (host copy for host_kmer_pack, device copy for the kernel); the slots are filled on the device
    std::vector<int32_t> h_slot; std::vector<uint32_t> h_off, h_len; std::vector<uint8_t> h_blob;
    int32_t *d_slot = nullptr; uint32_t *d_off = nullptr, *d_len = nullptr; uint8_t *d_blob = nullptr;
    ShKmerTable ht{}, dt{};
    // device copies of the slabs in the reader's hand
    struct Copy { uint8_t *d = nullptr; hipEvent_t up = nullptr; };
    std::atomic<size_t> buf_bytes{0};
    std::unordered_map<const char *, Copy> bound; std::vector<Copy> spare;
    // line table (buffer addresses, then records), rows and counts: pinned and device, grown on demand
    uint8_t *h_tab = nullptr, *d_tab = nullptr; size_t cap_tab = 0;
    uint32_t *h_rows = nullptr, *d_rows = nullptr; int32_t *h_counts = nullptr, *d_counts = nullptr; int64_t cap_rows = 0;
    hipEvent_t k0 = nullptr, k1 = nullptr; double kernel_ms = 0.0;
    int64_t lines_dev = 0, lines_host = 0, bytes_up = 0, launches = 0;
    // where the consumer's time goes (SEERHIP_DEBUG=host: one line on stderr when the reader closes), ns
    int64_t ns_in = 0, ns_out = 0, ns_pack = 0, ns_wait = 0;
    // ---- device inflate (inflate_api.inc; SEERHIP_ROUTE kmer_inflate=1): the decoding thread runs k_bgzf_inflate on a stream of its own and
    // leaves the slab's device copy in `inflated` for slab_in to bind; `mu` guards `spare` and `inflated`, which both threads touch
    std::mutex mu; std::unordered_map<const char *, Copy> inflated;
    hipStream_t istream = nullptr; hipEvent_t i0 = nullptr, i1 = nullptr;
    uint8_t *h_comp = nullptr, *d_comp = nullptr; size_t cap_comp = 0;       // the members' deflate bodies, one after the other
    uint8_t *h_mem = nullptr, *d_mem = nullptr; int64_t cap_mem = 0;         // [n] ShInfMember up; [n] status, [n] produced back
    std::atomic<int64_t> members_dev{0}, members_host{0};                    // (the consumer moves a member decoded again from one to the other)
    std::atomic<int64_t> infl_up{0}, infl_down{0}; std::atomic<double> infl_ms{0.0};      // (written by the decoding thread alone)
};
static bool kmer_inflate(void *self, char *buf, size_t pad, ShReaderMember *mem, int64_t n, std::string &err);      // inflate_api.inc

static inline int64_t kmer_now_ns() { return (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct KmerTimer { int64_t &acc; int64_t t0; explicit KmerTimer(int64_t &a) : acc(a), t0(kmer_now_ns()) {} ~KmerTimer() { acc += kmer_now_ns() - t0; } };

static bool kmer_hip(hipError_t e, const char *what, std::string &err)
{
    if (e == hipSuccess) return true;
    err = std::string("device k-mer reader: ") + what + ": " + hipGetErrorString(e);
    return false;
}

static char *kmer_alloc(void *self, size_t bytes)
{
    KmerDev *k = (KmerDev *)self;
    k->buf_bytes.store(bytes);
    if (!k->ctx) return (char *)malloc(bytes);
    void *p = nullptr;
    if (hipSetDevice(k->device) != hipSuccess || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return (char *)p;
}

static void kmer_release(void *self, char *buf)
{
    KmerDev *k = (KmerDev *)self;
    if (!k->ctx) { free(buf); return; }
    hipSetDevice(k->device);
    if (k->stream) hipStreamSynchronize(k->stream);        // (a reader closed early: its last uploads may still read the buffer)
    hipHostFree(buf);
}

// the device copy for the slab in `buf`: the one the inflate hook left for it, a spare one, or a new one
static bool kmer_copy_take(KmerDev *k, const char *buf, KmerDev::Copy &c, std::string &err)
{
    {
        std::lock_guard<std::mutex> lk(k->mu);
        const auto it = k->inflated.find(buf);
        if (it != k->inflated.end()) { c = it->second; k->inflated.erase(it); return true; }
        if (!k->spare.empty()) { c = k->spare.back(); k->spare.pop_back(); return true; }
    }
    if (!kmer_hip(hipMalloc((void **)&c.d, k->buf_bytes.load() + KMER_SLACK), "hipMalloc (slab)", err)) return false;
    if (!kmer_hip(hipEventCreateWithFlags(&c.up, hipEventDisableTiming), "hipEventCreate", err)) { hipFree(c.d); c.d = nullptr; return false; }
    return true;
}

static bool kmer_slab_in(void *self, const char *buf, size_t from, size_t to, std::string &err)
{
    KmerDev *k = (KmerDev *)self;
    // a second call for a slab in hand: a member of an inflated slab that the reader decoded again
    const auto again = k->bound.find(buf);
    if (again != k->bound.end()) { k->members_host += 1; k->members_dev -= 1; }
    if (!k->ctx) {                                         // (without a device only the inflate hook's slabs are kept track of, for that count)
        std::lock_guard<std::mutex> lk(k->mu);
        if (k->inflated.erase(buf)) k->bound[buf] = KmerDev::Copy();
        return true;
    }
    KmerTimer tm(k->ns_in);
    if (!kmer_hip(hipSetDevice(k->device), "hipSetDevice", err)) return false;
    KmerDev::Copy c;
    if (again != k->bound.end()) c = again->second;
    else if (!kmer_copy_take(k, buf, c, err)) return false;
    k->bound[buf] = c;
    if (to > from && !kmer_hip(hipMemcpyAsync(c.d + from, buf + from, to - from, hipMemcpyHostToDevice, k->stream), "hipMemcpyAsync (slab)", err)) return false;
    if (!kmer_hip(hipEventRecord(c.up, k->stream), "hipEventRecord", err)) return false;
    k->bytes_up += (int64_t)(to - from);
    return true;
}

static void kmer_slab_out(void *self, const char *buf)
{
    KmerDev *k = (KmerDev *)self;
    {                                                      // (a slab that failed before slab_in: what the inflate hook left for it)
        std::lock_guard<std::mutex> lk(k->mu);
        const auto left = k->inflated.find(buf);
        if (left != k->inflated.end()) { if (left->second.d) k->spare.push_back(left->second); k->inflated.erase(left); }
    }
    auto it = k->bound.find(buf);
    if (it == k->bound.end()) return;
    if (!k->ctx) { k->bound.erase(it); return; }
    KmerTimer tm(k->ns_out);
    hipSetDevice(k->device);
    hipEventSynchronize(it->second.up);                    // the pinned buffer is written again from here on
    { std::lock_guard<std::mutex> lk(k->mu); k->spare.push_back(it->second); }
    k->bound.erase(it);
}

static bool kmer_ensure(KmerDev *k, int64_t rows, size_t tab_bytes, std::string &err)
{
    if (rows > k->cap_rows) {
        const int64_t cap = std::max<int64_t>(rows, 4096);
        if (!kmer_hip(hipStreamSynchronize(k->stream), "hipStreamSynchronize", err)) return false;
        if (k->h_rows) hipHostFree(k->h_rows);
        if (k->h_counts) hipHostFree(k->h_counts);
        hipFree(k->d_rows); hipFree(k->d_counts);
        k->h_rows = k->d_rows = nullptr; k->h_counts = k->d_counts = nullptr; k->cap_rows = 0;
        if (!kmer_hip(hipHostMalloc((void **)&k->h_rows, (size_t)cap * k->row_words * 4, hipHostMallocDefault), "hipHostMalloc (rows)", err)) return false;
        if (!kmer_hip(hipHostMalloc((void **)&k->h_counts, (size_t)cap * 4, hipHostMallocDefault), "hipHostMalloc (counts)", err)) return false;
        if (!kmer_hip(dmalloc(&k->d_rows, (size_t)cap * k->row_words), "hipMalloc (rows)", err)) return false;
        if (!kmer_hip(dmalloc(&k->d_counts, (size_t)cap), "hipMalloc (counts)", err)) return false;
        k->cap_rows = cap;
    }
    if (tab_bytes > k->cap_tab) {
        const size_t cap = std::max<size_t>(tab_bytes * 2, (size_t)1 << 16);
        if (!kmer_hip(hipStreamSynchronize(k->stream), "hipStreamSynchronize", err)) return false;
        if (k->h_tab) hipHostFree(k->h_tab);
        hipFree(k->d_tab);
        k->h_tab = k->d_tab = nullptr; k->cap_tab = 0;
        if (!kmer_hip(hipHostMalloc((void **)&k->h_tab, cap, hipHostMallocDefault), "hipHostMalloc (line table)", err)) return false;
        if (!kmer_hip(hipMalloc((void **)&k->d_tab, cap), "hipMalloc (line table)", err)) return false;
        k->cap_tab = cap;
    }
    return true;
}

// a row of row_words words into the caller's row of row_bytes bytes (zeroed by the reader)
static inline void kmer_put_row(uint8_t *dst, int64_t row_bytes, const uint32_t *row, int row_words)
{
    memcpy(dst, row, (size_t)std::min<int64_t>(row_bytes, (int64_t)row_words * 4));
}

static bool kmer_pack(void *self, const ShReaderLine *lines, int64_t n, uint8_t *bits, int64_t row_bytes, int32_t *counts, std::string &err)
{
    KmerDev *k = (KmerDev *)self;
    KmerTimer tm(k->ns_pack);
    std::vector<int64_t> host_rows;                        // lines the kernel does not see
    int64_t n_dev = 0;
    if (k->ctx) {
        if (!kmer_hip(hipSetDevice(k->device), "hipSetDevice", err)) return false;
        // the buffers of this call, in the order the lines meet them
        std::vector<uint64_t> bases;
        std::vector<uint32_t> slab_of((size_t)n, 0xffffffffu);
        const char *last_buf = nullptr;
        for (int64_t v = 0; v < n; ++v) {
            const ShReaderLine &ln = lines[v];
            const auto it = ln.buf ? k->bound.find(ln.buf) : k->bound.end();
            if (it == k->bound.end() || (uint64_t)(ln.p - ln.buf) + ln.len >= 0xfffffff0ull) { host_rows.push_back(v); continue; }
            if (ln.buf != last_buf) { bases.push_back((uint64_t)(uintptr_t)it->second.d); last_buf = ln.buf; }
            slab_of[(size_t)v] = (uint32_t)(bases.size() - 1);
            ++n_dev;
        }
        if (n_dev) {
            const size_t tab_bytes = bases.size() * 8 + (size_t)n_dev * sizeof(ShKmerRec);
            if (!kmer_ensure(k, n, tab_bytes, err)) return false;
            memcpy(k->h_tab, bases.data(), bases.size() * 8);
            ShKmerRec *recs = (ShKmerRec *)(k->h_tab + bases.size() * 8);
            int64_t j = 0;
            for (int64_t v = 0; v < n; ++v) {
                if (slab_of[(size_t)v] == 0xffffffffu) continue;
                ShKmerRec r; r.off = (uint32_t)(lines[v].p - lines[v].buf); r.len = (uint32_t)lines[v].len; r.slab = slab_of[(size_t)v]; r.row = (uint32_t)v;
                recs[j++] = r;
            }
            if (!kmer_hip(hipMemcpyAsync(k->d_tab, k->h_tab, tab_bytes, hipMemcpyHostToDevice, k->stream), "hipMemcpyAsync (line table)", err)) return false;
            if (!kmer_hip(hipEventRecord(k->k0, k->stream), "hipEventRecord", err)) return false;
            if (!kmer_hip(shk_kmer_pack(k->stream, (const uint64_t *)k->d_tab, (const ShKmerRec *)(k->d_tab + bases.size() * 8), n_dev, k->dt, k->row_words,
                                        k->d_rows, k->d_counts), "k_kmer_pack", err)) return false;
            if (!kmer_hip(hipEventRecord(k->k1, k->stream), "hipEventRecord", err)) return false;
            // (rows of lines the kernel did not see are not written: they are not read below either)
            if (!kmer_hip(hipMemcpyAsync(k->h_rows, k->d_rows, (size_t)n * k->row_words * 4, hipMemcpyDeviceToHost, k->stream), "hipMemcpyAsync (rows)", err)) return false;
            if (!kmer_hip(hipMemcpyAsync(k->h_counts, k->d_counts, (size_t)n * 4, hipMemcpyDeviceToHost, k->stream), "hipMemcpyAsync (counts)", err)) return false;
            { KmerTimer tw(k->ns_wait); if (!kmer_hip(hipStreamSynchronize(k->stream), "hipStreamSynchronize", err)) return false; }
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, k->k0, k->k1) == hipSuccess) k->kernel_ms += (double)ms;
            k->launches += 1; k->lines_dev += n_dev;
            if (row_bytes == (int64_t)k->row_words * 4 && host_rows.empty()) memcpy(bits, k->h_rows, (size_t)n * (size_t)row_bytes);
            else for (int64_t v = 0; v < n; ++v) if (slab_of[(size_t)v] != 0xffffffffu) kmer_put_row(bits + (size_t)v * row_bytes, row_bytes, k->h_rows + (size_t)v * k->row_words, k->row_words);
            for (int64_t v = 0; v < n; ++v) if (slab_of[(size_t)v] != 0xffffffffu) counts[v] = k->h_counts[v];
        }
    } else {
        host_rows.resize((size_t)n);
        for (int64_t v = 0; v < n; ++v) host_rows[(size_t)v] = v;
    }
    if (!host_rows.empty()) {
        const std::function<void(int64_t)> fn = [&](int64_t i) {
            static thread_local std::vector<uint32_t> row;
            row.resize((size_t)k->row_words);
            const int64_t v = host_rows[(size_t)i];
            host_kmer_pack(lines[v].p, lines[v].len, k->ht, row.data(), k->row_words, counts + v);
            kmer_put_row(bits + (size_t)v * row_bytes, row_bytes, row.data(), k->row_words);
        };
        shost::pool().run((int64_t)host_rows.size(), 8, fn, shost::ST_READER_PARSE);
        k->lines_host += (int64_t)host_rows.size();
    }
    return true;
}

static void kmer_destroy(void *self)
{
    KmerDev *k = (KmerDev *)self;
    if (k->ctx && sh_debug("host"))
        fprintf(stderr, "[reader debug] device route: %lld lines in %lld launches, %.1f MB of text up; the consumer spent %.3f s queueing slab uploads, %.3f s waiting for them "
                        "before a slab was let go, %.3f s in the calls' tokenising (of it %.3f s waiting for the stream: upload, kernel %.3f s, rows back)\n",
                (long long)k->lines_dev, (long long)k->launches, (double)k->bytes_up * 1e-6, (double)k->ns_in * 1e-9, (double)k->ns_out * 1e-9, (double)k->ns_pack * 1e-9,
                (double)k->ns_wait * 1e-9, k->kernel_ms * 1e-3);
    if (k->ctx) {
        hipSetDevice(k->device);
        if (k->stream) hipStreamSynchronize(k->stream);
        if (k->istream) hipStreamSynchronize(k->istream);
        for (auto &b : k->bound) k->spare.push_back(b.second);
        for (auto &b : k->inflated) k->spare.push_back(b.second);
        if (k->h_comp) hipHostFree(k->h_comp);
        if (k->h_mem) hipHostFree(k->h_mem);
        hipFree(k->d_comp); hipFree(k->d_mem);
        if (k->i0) hipEventDestroy(k->i0);
        if (k->i1) hipEventDestroy(k->i1);
        if (k->istream) hipStreamDestroy(k->istream);
        for (auto &c : k->spare) { hipFree(c.d); if (c.up) hipEventDestroy(c.up); }
        if (k->h_tab) hipHostFree(k->h_tab);
        if (k->h_rows) hipHostFree(k->h_rows);
        if (k->h_counts) hipHostFree(k->h_counts);
        hipFree(k->d_tab); hipFree(k->d_rows); hipFree(k->d_counts);
        hipFree(k->d_slot); hipFree(k->d_off); hipFree(k->d_len); hipFree(k->d_blob);
        if (k->k0) hipEventDestroy(k->k0);
        if (k->k1) hipEventDestroy(k->k1);
        if (k->stream) hipStreamDestroy(k->stream);
    }
    delete k;
}

// the table of `names`: serially on the host (first occurrence wins), and with a context a second time by k_kmer_table_build
static int kmer_build_table(KmerDev *k, const char *const *names, int n)
{
    uint32_t cap = 16; while (cap < (uint32_t)n * 4u) cap <<= 1;
    const uint32_t mask = cap - 1;
    k->h_off.resize((size_t)n); k->h_len.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        const size_t len = strlen(names[i]);
        if (k->h_blob.size() + len >= 0xffffffffull) return fail(SH_EINVAL, "sample names of 4 GB or more");
        k->h_off[(size_t)i] = (uint32_t)k->h_blob.size(); k->h_len[(size_t)i] = (uint32_t)len;
        k->h_blob.insert(k->h_blob.end(), (const uint8_t *)names[i], (const uint8_t *)names[i] + len);
    }
    k->h_blob.push_back(0);                                 // (never empty)
    k->h_slot.assign(cap, -1);
    k->ht.slot = k->h_slot.data(); k->ht.name_off = k->h_off.data(); k->ht.name_len = k->h_len.data(); k->ht.blob = k->h_blob.data(); k->ht.mask = mask;
    for (int i = 0; i < n; ++i) {
        const uint8_t *s = k->h_blob.data() + k->h_off[(size_t)i];
        uint32_t h = KMER_HASH_INIT;
        for (uint32_t j = 0; j < k->h_len[(size_t)i]; ++j) h = shk_kmer_hash_step(h, s[j]);
        if (shk_kmer_find(k->ht, s, k->h_len[(size_t)i], h) >= 0) continue;
        uint32_t at = h & mask;
        while (k->h_slot[at] >= 0) at = (at + 1) & mask;
        k->h_slot[at] = i;
    }
    if (!k->ctx) return SH_OK;
    HIPCHK(dmalloc(&k->d_slot, (size_t)cap)); HIPCHK(dmalloc(&k->d_off, (size_t)n)); HIPCHK(dmalloc(&k->d_len, (size_t)n)); HIPCHK(dmalloc(&k->d_blob, k->h_blob.size()));
    HIPCHK(hipMemsetAsync(k->d_slot, 0xFF, (size_t)cap * 4, k->stream));
    HIPCHK(hipMemcpyAsync(k->d_off, k->h_off.data(), (size_t)n * 4, hipMemcpyHostToDevice, k->stream));
    HIPCHK(hipMemcpyAsync(k->d_len, k->h_len.data(), (size_t)n * 4, hipMemcpyHostToDevice, k->stream));
    HIPCHK(hipMemcpyAsync(k->d_blob, k->h_blob.data(), k->h_blob.size(), hipMemcpyHostToDevice, k->stream));
    HIPCHK(shk_kmer_table_build(k->stream, k->d_slot, mask, k->d_off, k->d_len, k->d_blob, n));
    HIPCHK(hipStreamSynchronize(k->stream));                // (the host vectors are pageable)
    k->dt.slot = k->d_slot; k->dt.name_off = k->d_off; k->dt.name_len = k->d_len; k->dt.blob = k->d_blob; k->dt.mask = mask;
    return SH_OK;
}

static int kmer_open_device(KmerDev *k)
{
    HIPCHK(hipSetDevice(k->device));
    HIPCHK(hipStreamCreateWithFlags(&k->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&k->k0)); HIPCHK(hipEventCreate(&k->k1));
    return SH_OK;
}

// what sh_reader_set_inflate asked of the calling thread's next sh_reader_open_dev: -1 as the route key says, 0 off, 1 on
static thread_local int g_kmer_inflate = -1;
void sh_reader_set_inflate(int on) { g_kmer_inflate = on < 0 ? -1 : (on ? 1 : 0); }

sh_reader *sh_reader_open_dev(sh_ctx *ctx, const char *path, const char *const *sample_names, int n_samples)
{
    const int asked = g_kmer_inflate;
    g_kmer_inflate = -1;                                   // (it holds for one open, whatever becomes of it)
    auto refuse = [](int code, const std::string &msg) -> sh_reader * { fail(code, msg); sh_reader_set_error(msg.c_str()); return nullptr; };
    if (!path || !sample_names || n_samples < 1) return refuse(SH_EINVAL, "bad argument");
    if (ctx && ctx->N != n_samples) return refuse(SH_ESHAPE, "the context was created for another number of samples");
    const int row_words = (n_samples + 31) / 32;
    // (the row and a few words beside it in 64 KB of LDS: 16 352 words)
    if (ctx && shk_kmer_lds_bytes(row_words) + 128 > 65536) return refuse(SH_ESHAPE, "too many samples for the k-mer kernel's row in LDS (at most 523 264)");
    KmerDev *k = new KmerDev();
    k->ctx = ctx; k->device = ctx ? ctx->device : 0; k->N = n_samples; k->row_words = row_words;
    if ((ctx && kmer_open_device(k) != SH_OK) || kmer_build_table(k, sample_names, n_samples) != SH_OK) {
        const std::string keep = g_err; kmer_destroy(k); return refuse(SH_EHIP, keep);
    }
    ShReaderHooks h;
    h.self = k; h.alloc = kmer_alloc; h.release = kmer_release; h.slab_in = kmer_slab_in; h.slab_out = kmer_slab_out; h.pack = kmer_pack; h.destroy = kmer_destroy;
    // SEERHIP_ROUTE kmer_inflate=1, or sh_reader_set_inflate before this call on this thread: the members of a BGZF file are decoded by
    // k_bgzf_inflate (without a context: by the host build of its core)
    const char *ki = sh_route("kmer_inflate");
    if (asked == 1 || (asked < 0 && ki && std::string(ki) == "1")) h.inflate = kmer_inflate;
    sh_reader *r = sh_reader_open_hooked(path, sample_names, n_samples, h);      // (owns k from here on)
    if (!r) fail(SH_EINVAL, sh_reader_error());
    return r;
}

int sh_reader_dev_stats(sh_reader *r, int64_t *lines_dev, int64_t *lines_host, int64_t *bytes_up, int64_t *launches)
{
    KmerDev *k = (KmerDev *)sh_reader_hooks_self(r);
    if (!k) return fail(SH_EINVAL, "not a reader opened by sh_reader_open_dev");
    if (lines_dev) *lines_dev = k->lines_dev;
    if (lines_host) *lines_host = k->lines_host;
    if (bytes_up) *bytes_up = k->bytes_up;
    if (launches) *launches = k->launches;
    return SH_OK;
}

double sh_reader_dev_kernel_ms(sh_reader *r)
{
    KmerDev *k = (KmerDev *)sh_reader_hooks_self(r);
    return k ? k->kernel_ms : -1.0;
}
