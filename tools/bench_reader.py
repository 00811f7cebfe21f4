"""Throughput of the native k-mer reader (csrc/reader.cpp) on a synthetic k-mer file, N samples x V k-mers, by container:
plain text, gzip through zlib's gzread (SEERHIP_ROUTE reader=zlib, the round-1 path), gzip through the in-tree inflate on one thread
(SEERHIP_ROUTE reader=serial) and on several (the default, csrc/inflate_par.h), BGZF (member-parallel).
No GPU involved; run it on the GPU host to see what feeds the engine there.  Prints one JSON line.

--device: the same generated file (N = 5000; 40 000 k-mers unless V says otherwise) through the host route (sh_reader_open) and the device route
(sh_reader_open_dev, k_kmer_pack) alternately in ONE process, for plain text, gzip and BGZF: a warm-up pass of each, then 3 passes of each; the
medians, the spread of the host passes (the yardstick, timed in the same run), the device route's counters and the kernel's own time (events).
Every pass of either route is checked against the first pass's carrier count.

--inflate: the same file as BGZF only (N = 5000, 40 000 k-mers: 1.5 GB of text) through three routes alternately in ONE process: the host route,
the device route (--device-reader) and the device route with the device inflate (--device-inflate: k_bgzf_inflate, SEERHIP_ROUTE kmer_inflate=1).
A warm-up pass of each, then 3 passes of each; per route the median and the spread, compared with the host route of the same run; of the
device inflate also the kernel's own time by stream events (ms, and GB/s of text produced), bytes up and down, members decoded on the
device and on the host.  The gzip file is not written in this mode."""
import gzip, json, os, struct, sys, time, zlib
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyseer_amd.input import NativeKmerReader

INFLATE = "--inflate" in sys.argv[1:]
DEVICE = "--device" in sys.argv[1:]
N = int(os.environ.get("N", 5000)); V = int(os.environ.get("V", 40000 if DEVICE or INFLATE else 12000)); BS = int(os.environ.get("BLOCK", 4096))
d = os.environ.get("OUT", "/tmp/rb"); os.makedirs(d, exist_ok=True)
rng = np.random.default_rng(0)
names = ["sample_%05d" % i for i in range(N)]
tok = np.array([n + ":1" for n in names], dtype=object)
t0 = time.time()
META = [N, V] + (["bgzf only"] if INFLATE else [])
if os.environ.get("REUSE") and os.path.exists(d + "/k.bgzf.gz") and os.path.exists(d + "/meta.json") and json.load(open(d + "/meta.json")) in ([N, V], META):
    text = open(d + "/k.txt", "rb").read()                     # REUSE=1: the files of an earlier run with the same N, V
else:
    parts = []
    for v in range(V):
        af = rng.uniform(0.02, 0.98)
        idx = np.nonzero(rng.random(N) < af)[0]
        parts.append("".join(rng.choice(list("ACGT"), 31)) + " | " + " ".join(tok[idx]) + "\n")
        if INFLATE and v % 5000 == 4999: sys.stderr.write("generated %d k-mers\n" % (v + 1)); sys.stderr.flush()
    text = "".join(parts).encode(); del parts
    open(d + "/k.txt", "wb").write(text)
    if not INFLATE:                                            # (--inflate reads BGZF only: no gzip file)
        co = zlib.compressobj(6, zlib.DEFLATED, 31)
        with open(d + "/k.gz", "wb") as f:
            for i in range(0, len(text), 1 << 24):
                f.write(co.compress(text[i:i + (1 << 24)]))
            f.write(co.flush())
    with open(d + "/k.bgzf.gz", "wb") as f:
        for i in range(0, len(text), 65280):
            ch = text[i:i + 65280]
            c = zlib.compressobj(6, zlib.DEFLATED, -15); comp = c.compress(ch) + c.flush()
            f.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 12 + 6 + len(comp) + 8 - 1))
            f.write(comp + struct.pack("<II", zlib.crc32(ch) & 0xFFFFFFFF, len(ch)))
    json.dump(META, open(d + "/meta.json", "w"))
gen = time.time() - t0
res = {"n_samples": N, "kmers": V, "text_MB": len(text) / 1e6, "cores": os.cpu_count(), "generate_s": gen}
if not INFLATE: res["gz_MB"] = os.path.getsize(d + "/k.gz") / 1e6
if INFLATE:
    from pyseer_amd.engine import Engine
    eng = Engine(N)
    PASSES = int(os.environ.get("REPS", 3))
    path = d + "/k.bgzf.gz"
    ROUTES = (("host", None, None), ("device_reader", eng, False), ("device_inflate", eng, True))

    def one_pass(engine, inflate):
        t0 = time.time(); tot = 0; cs = 0
        r = NativeKmerReader(path, names, BS, engine=engine, inflate=inflate)
        for bits, counts, blob, off in r.raw_blocks():
            tot += counts.shape[0]; cs += int(counts.sum())
        st = dict(r.dev_stats(), inflate=r.inflate_stats()) if engine is not None else None
        r.close()
        assert tot == V
        return time.time() - t0, cs, st
    want_cs = one_pass(None, None)[1]                          # warm-up passes (page cache, pinned memory, the module's kernels)
    for _, engine, inflate in ROUTES[1:]:
        assert one_pass(engine, inflate)[1] == want_cs
    times = {tag: [] for tag, _, _ in ROUTES}; stats = {}
    for rep in range(PASSES):
        for tag, engine, inflate in ROUTES:
            t, cs, st = one_pass(engine, inflate); assert cs == want_cs, (tag, cs, want_cs)
            times[tag].append(t); stats[tag] = st
    mh = float(np.median(times["host"]))
    res["bgzf_MB"] = os.path.getsize(path) / 1e6
    for tag, _, _ in ROUTES:
        t = times[tag]; m = float(np.median(t))
        res[tag] = {"kmers_per_s": V / m, "min_max_kmers_per_s": [V / max(t), V / min(t)], "pass_s": t, "over_host": mh / m, "stats": stats[tag]}
        sys.stderr.write("%-14s %7.0f k-mers/s (passes %.0f .. %.0f)   x%.2f of the host route\n" % (tag, V / m, V / max(t), V / min(t), mh / m))
    inf = stats["device_inflate"]["inflate"]
    res["k_bgzf_inflate"] = {"ms_per_pass": inf["kernel_ms"], "text_GB_per_s": len(text) / 1e9 / (inf["kernel_ms"] * 1e-3) if inf["kernel_ms"] > 0 else None,
                             "bytes_up": inf["bytes_up"], "bytes_down": inf["bytes_down"], "text_bytes_up": stats["device_inflate"]["bytes_up"],
                             "members_dev": inf["members_dev"], "members_host": inf["members_host"]}
    sys.stderr.write("k_bgzf_inflate %.1f ms per pass (%.2f GB/s of text), %.0f MB up, %.0f MB down, %.0f MB of text up, members on the device %d / on the host %d\n"
                     % (inf["kernel_ms"], len(text) / 1e6 / max(inf["kernel_ms"], 1e-9), inf["bytes_up"] / 1e6, inf["bytes_down"] / 1e6,
                        stats["device_inflate"]["bytes_up"] / 1e6, inf["members_dev"], inf["members_host"]))
    eng.close()
    res["block"] = BS; res["passes"] = PASSES
    print(json.dumps(res)); sys.exit(0)
if DEVICE:
    from pyseer_amd.engine import Engine
    eng = Engine(N)
    PASSES = int(os.environ.get("REPS", 3))

    def one_pass(path, engine):
        t0 = time.time(); tot = 0; cs = 0
        r = NativeKmerReader(path, names, BS, engine=engine)
        for bits, counts, blob, off in r.raw_blocks():
            tot += counts.shape[0]; cs += int(counts.sum())
        st = r.dev_stats() if engine is not None else None
        r.close()
        assert tot == V
        return time.time() - t0, cs, st
    for tag, path in (("plain", "k.txt"), ("gzip", "k.gz"), ("bgzf", "k.bgzf.gz")):
        path = d + "/" + path
        _, want_cs, _ = one_pass(path, None)                   # warm-up passes (page cache, pinned memory, the module's kernels)
        _, cs, _ = one_pass(path, eng)
        assert cs == want_cs, (tag, cs, want_cs)
        th, td, st = [], [], None
        for rep in range(PASSES):
            t, cs, _ = one_pass(path, None); assert cs == want_cs; th.append(t)
            t, cs, st = one_pass(path, eng); assert cs == want_cs; td.append(t)
        mh, md = float(np.median(th)), float(np.median(td))
        res[tag] = {"host_kmers_per_s": V / mh, "host_min_max_kmers_per_s": [V / max(th), V / min(th)], "device_kmers_per_s": V / md,
                    "device_min_max_kmers_per_s": [V / max(td), V / min(td)], "device_over_host": mh / md, "dev_stats": st,
                    "kernel_share_of_pass": st["kernel_ms"] * 1e-3 / td[-1]}
        sys.stderr.write("%-5s host %7.0f k-mers/s (passes %.0f .. %.0f)   device %7.0f k-mers/s (passes %.0f .. %.0f)   x%.2f   kernel %.1f ms of the last %.0f ms pass, "
                         "%d launches, %.0f MB up, lines on the device %d / on the host %d\n"
                         % (tag, V / mh, V / max(th), V / min(th), V / md, V / max(td), V / min(td), mh / md, st["kernel_ms"], td[-1] * 1e3, st["launches"],
                            st["bytes_up"] / 1e6, st["lines_dev"], st["lines_host"]))
    eng.close()
    res["block"] = BS; res["passes"] = PASSES
    print(json.dumps(res)); sys.exit(0)
want = None
TAGS = os.environ.get("TAGS", "").split(",") if os.environ.get("TAGS") else None
for tag, path, env in (("plain", "k.txt", None), ("gzip_zlib", "k.gz", "zlib"), ("gzip_fast", "k.gz", "serial"), ("gzip_par", "k.gz", None), ("bgzf", "k.bgzf.gz", None)):
    if TAGS and tag not in TAGS: continue
    base = ",".join(it for it in os.environ.get("SEERHIP_ROUTE", "").split(",") if it and not it.startswith("reader="))
    route = ",".join(x for x in (base, "reader=" + env if env else "") if x)
    if route: os.environ["SEERHIP_ROUTE"] = route
    else: os.environ.pop("SEERHIP_ROUTE", None)
    best = 0.0
    for rep in range(int(os.environ.get("REPS", 2))):
        t0 = time.time(); tot = 0; cs = 0
        for bits, counts, blob, off in NativeKmerReader(d + "/" + path, names, BS).raw_blocks():
            tot += counts.shape[0]; cs += int(counts.sum())
        dt = time.time() - t0
        best = max(best, tot / dt)
        assert tot == V
        if want is None: want = cs
        assert cs == want, (tag, cs, want)
    res[tag + "_kmers_per_s"] = best; res[tag + "_text_MBps"] = best * len(text) / V / 1e6
if TAGS:
    res["route"] = os.environ.get("SEERHIP_ROUTE")
    print(json.dumps(res)); sys.exit(0)
# the same gzip text cut into NF files at line boundaries and read as one stream (--kmers a.gz b.gz ...): one reader thread per file
import pandas as pd
from pyseer_amd.input import iter_packed_blocks_native_multi
NF = int(os.environ.get("FILES", 4))
lines = text.splitlines(True)
paths = []
for i in range(NF):
    path = d + "/part%d.gz" % i
    open(path, "wb").write(gzip.compress(b"".join(lines[i * len(lines) // NF:(i + 1) * len(lines) // NF]), 6))
    paths.append(path)
ph = pd.Series(np.zeros(N), index=names)
best = 0.0
for rep in range(2):
    t0 = time.time(); tot = 0
    for blk in iter_packed_blocks_native_multi(ph, paths, 0.0, 1.0, BS):
        tot += len(blk.names)
    best = max(best, tot / (time.time() - t0))
    assert tot == V
res["gzip_fast_%d_files_kmers_per_s" % NF] = best
from pyseer_amd.input import iter_packed_blocks_native
best = 0.0
for rep in range(2):                                        # the single file through the same block construction (AF filter, names), for comparison
    t0 = time.time(); tot = 0
    for blk in iter_packed_blocks_native(ph, d + "/k.gz", 0.0, 1.0, BS):
        tot += len(blk.names)
    best = max(best, tot / (time.time() - t0))
res["gzip_fast_1_file_blocks_kmers_per_s"] = best
print(json.dumps(res))
