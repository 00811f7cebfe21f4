"""Rates of the VCF readers on a generated call set: N = 5000 phenotyped samples among 5200 columns (tests/_vcf_text.py: 1-byte and 20-byte
sample fields, GT first or second in FORMAT, ~3 % missing, multi-allelic and filtered records), tiled to at least --gb of text, BGZF.

  python tools/bench_vcf_reader.py --dir /tmp/vcfbench --gb 1.0                       # (a) Python reader, (b) native end to end, (d) host tokeniser
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_vcf_reader.py --dir /tmp/vcfbench --gb 1.0 --only native
  python tools/bench_vcf_reader.py --kernel-stats OUT                                 # (c) k_vcf_gt_pack alone, from the trace of the run above

(b) and (d) read the whole file twice and report the second pass (the first pass also pays the page cache and the pinned slabs); (a) reads the
first --python-records records.  (d) is the same reader with the kernel's work done by shvcf::host_gt_pack on the host pool (16 threads under
the GPU host's quota).  Prints one JSON line per measurement.

  python tools/bench_vcf_reader.py --bcf --dir /tmp/vcfbench --records 200000         # BCF against the text BGZF of the same records
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_vcf_reader.py --bcf --dir /tmp/vcfbench --records 200000 --only native
  python tools/bench_vcf_reader.py --bcf --kernel-stats OUT --records 200000          # k_bcf_gt_pack and k_vcf_gt_pack alone, from that trace

--bcf writes the same generated records twice -- gen.vcf.gz as above and gen.bcf (tests/_bcf_bytes.py; 2000 records converted, their BGZF
members tiled) -- and reads both in one run, the two formats alternating: one warm-up pass each, then three timed passes each, the median
reported.  Per format: end to end (inflate, framing, fixed fields, copy into the pinned slabs, H2D, kernel, rows back), the host half alone
(ctx == NULL and no sample phenotyped: inflate, framing, fixed fields and the copy of what would go to the device, no call reduced; for text
the host pool still finds the column tabs), and the bytes sent to the device per record (sh_vcf_stats)."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12          # bytes/s: float4 copy measured, and the specification


def make_file(d, gb, records=None):
    """gen.vcf.gz (BGZF) of at least `gb` GB of text -- or, with `records`, of at least that many records --, first.vcf (its first 2000 records
    as plain text) and meta.json under d; (path, meta)."""
    from _vcf_text import bgzf_bytes, generated_vcf
    os.makedirs(d, exist_ok=True)
    path, meta = os.path.join(d, "gen.vcf.gz"), os.path.join(d, "meta.json")
    if records is not None:
        gb = "%d records" % records
    if os.path.exists(path) and os.path.exists(meta) and json.load(open(meta))["gb"] == gb:
        return path, json.load(open(meta))
    text, pheno, cols = generated_vcf(n_pheno=5000, n_cols=5200, n_records=2000, seed=7, missing=0.03)
    head_end = text.index(b"\n", text.index(b"#CHROM")) + 1
    body = text[head_end:]
    tiles = max(1, -(-records // 2000)) if records is not None else max(1, int(-(-gb * 1e9 // len(body))))
    with open(path, "wb") as f:
        f.write(bgzf_bytes(text[:head_end], level=1)[:-28])
        comp = bgzf_bytes(body, level=1)[:-28]                   # (without the end-of-file member)
        for _ in range(tiles):
            f.write(comp)
        f.write(bgzf_bytes(b"")[-28:])
    with open(os.path.join(d, "first.vcf"), "wb") as f:
        f.write(text)
    m = {"gb": gb, "records": 2000 * tiles, "text_bytes": head_end + tiles * len(body), "file_bytes": os.path.getsize(path), "samples": pheno}
    json.dump(m, open(meta, "w"))
    return path, m


def kernel_stats(out_dir, kernel="k_vcf_gt_pack"):
    rows = []
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    for r in rows:
        if kernel in r["Name"]:
            return {"kernel": kernel, "calls": int(r["Calls"]), "total_s": float(r["TotalDurationNs"]) * 1e-9, "mean_us": float(r["AverageNs"]) * 1e-3}
    raise SystemExit("no %s row under %s" % (kernel, out_dir))


def make_bcf_file(d, records):
    """gen.bcf next to make_file's gen.vcf.gz: the same 2000 generated records as BCF, their BGZF members tiled as often; (path, file bytes)."""
    import struct
    from _bcf_bytes import bcf_from_vcf_text
    from _vcf_text import bgzf_bytes, generated_vcf
    path, tiles = os.path.join(d, "gen.bcf"), max(1, -(-records // 2000))
    stamp = os.path.join(d, "bcf_meta.json")
    if not (os.path.exists(path) and os.path.exists(stamp) and json.load(open(stamp))["tiles"] == tiles):
        text = generated_vcf(n_pheno=5000, n_cols=5200, n_records=2000, seed=7, missing=0.03)[0]
        raw = bcf_from_vcf_text(text, container=False)
        head_end = 9 + struct.unpack("<I", raw[5:9])[0]
        with open(path, "wb") as f:
            f.write(bgzf_bytes(raw[:head_end], level=1)[:-28])
            comp = bgzf_bytes(raw[head_end:], level=1)[:-28]
            for _ in range(tiles):
                f.write(comp)
            f.write(bgzf_bytes(b"")[-28:])
        json.dump({"tiles": tiles, "decoded_bytes": head_end + tiles * (len(raw) - head_end)}, open(stamp, "w"))
    return path, os.path.getsize(path), json.load(open(stamp))["decoded_bytes"]


def one_pass(path, samples, eng, block):
    from pyseer_amd.input import NativeVcfReader
    r = NativeVcfReader(path, samples, eng, block)
    t0 = time.perf_counter()
    n = npres = nmiss = 0
    for rb in r.raw_blocks():                                            # (sh_vcf_next ends in a stream synchronise)
        n += len(rb["skip"]); npres += int(rb["n_present"].sum()); nmiss += int(rb["n_missing"].sum())
    dt = time.perf_counter() - t0
    st = r.stats()
    r.close()
    return dt, n, npres, nmiss, st


def bench_bcf(o):
    import statistics
    text_path, meta = make_file(o.dir, o.gb, o.records)
    bcf_path, bcf_bytes, bcf_decoded = make_bcf_file(o.dir, meta["records"])
    samples = meta["samples"]
    paths = {"bcf": bcf_path, "text": text_path}
    print(json.dumps({"what": "inputs", "records": meta["records"], "n_samples": len(samples), "columns": 5200, "text_GB": meta["text_bytes"] / 1e9,
                      "text_bgzf_MB": meta["file_bytes"] / 1e6, "bcf_GB": bcf_decoded / 1e9, "bcf_bgzf_MB": bcf_bytes / 1e6, "block": o.block}))
    res = {}
    for stage in ("end_to_end", "host_half_alone"):
        if o.only == "native" and stage != "end_to_end":
            continue
        eng = None
        who = samples
        if stage == "end_to_end":
            from pyseer_amd.engine import Engine
            eng = Engine(len(samples))
        else:
            who = ["no such sample"]
        times = {"bcf": [], "text": []}
        for rep in range(1 + o.repeats):                                 # pass 0 warms up: page cache, pinned slabs, code objects
            for fmt in ("bcf", "text"):
                dt, n, npres, nmiss, st = one_pass(paths[fmt], who, eng, o.block)
                assert n == meta["records"], (n, meta["records"])
                if rep:
                    times[fmt].append(dt)
                res[(stage, fmt)] = {"present_calls": npres, "missing_calls": nmiss, "bytes_to_device_per_record": st["sample_bytes"] / n, "launches": st["launches"]}
        if eng is not None:
            eng.close()
            assert res[(stage, "bcf")]["present_calls"] == res[(stage, "text")]["present_calls"] and res[(stage, "bcf")]["missing_calls"] == res[(stage, "text")]["missing_calls"]
        for fmt in ("bcf", "text"):
            med = statistics.median(times[fmt])
            r = dict(res[(stage, fmt)], what=stage, format=fmt, passes_s=times[fmt], median_s=med, records_per_s=meta["records"] / med)
            if eng is None:
                del r["bytes_to_device_per_record"], r["launches"], r["present_calls"], r["missing_calls"]
            print(json.dumps(r))
            res[(stage, fmt)] = r
        print(json.dumps({"what": stage + ", BCF over text", "ratio_of_rates": res[(stage, "bcf")]["records_per_s"] / res[(stage, "text")]["records_per_s"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/vcfbench")
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--only", default=None, choices=["python", "native", "host"])
    ap.add_argument("--python-records", type=int, default=400)
    ap.add_argument("--block", type=int, default=3000)
    ap.add_argument("--bcf", action="store_true", help="BCF against the text BGZF of the same records, in one run")
    ap.add_argument("--records", type=int, default=None, help="with --bcf: records of both files (tiles of 2000)")
    ap.add_argument("--repeats", type=int, default=3, help="with --bcf: timed passes per format after the warm-up pass")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--traced-json", default=None, help="with --kernel-stats: the JSON line the traced run printed (its sample bytes, two passes)")
    o = ap.parse_args()
    if o.bcf and o.kernel_stats:                                         # the traced --bcf --only native run: (1 + repeats) passes per format
        for kernel in ("k_bcf_gt_pack", "k_vcf_gt_pack"):
            k = kernel_stats(o.kernel_stats, kernel)
            k["records"] = (1 + o.repeats) * (o.records or 0)
            if k["records"]:
                k["records_per_s"] = k["records"] / k["total_s"]
            print(json.dumps(k))
        return
    if o.bcf:
        bench_bcf(o)
        return
    if o.kernel_stats:
        k = kernel_stats(o.kernel_stats)
        if o.traced_json:
            line = json.loads(open(o.traced_json).read().strip().splitlines()[-1])
            k["sample_bytes"] = 2 * line["sample_bytes"]                 # the traced run reads the file twice
            k["records"] = 2 * line["records"]
            k["records_per_s"] = k["records"] / k["total_s"]
            k["bytes_per_s"] = k["sample_bytes"] / k["total_s"]
            k["share_of_measured_hbm_copy_rate"] = k["bytes_per_s"] / HBM_MEASURED
            k["share_of_hbm_spec"] = k["bytes_per_s"] / HBM_SPEC
        print(json.dumps(k))
        return
    path, meta = make_file(o.dir, o.gb)
    samples = meta["samples"]
    base = {"records": meta["records"], "text_GB": meta["text_bytes"] / 1e9, "file_MB": meta["file_bytes"] / 1e6, "n_samples": len(samples), "columns": 5200}
    if o.only in (None, "python"):
        import contextlib
        import io
        from pyseer_amd.input import VcfFile
        f = VcfFile(os.path.join(o.dir, "first.vcf"))
        t0 = time.perf_counter()
        n = 0
        with contextlib.redirect_stderr(io.StringIO()):
            for rec in f:
                f.apply(rec, {})
                n += 1
                if n >= o.python_records:
                    break
        dt = time.perf_counter() - t0
        print(json.dumps(dict(base, reader="python (plain text, first %d records)" % n, seconds=dt, records_per_s=n / dt)))
    for which in ("native", "host"):
        if o.only not in (None, which):
            continue
        from pyseer_amd.input import NativeVcfReader
        eng = None
        if which == "native":
            from pyseer_amd.engine import Engine
            eng = Engine(len(samples))
        for rep in range(2):
            r = NativeVcfReader(path, samples, eng, o.block)
            t0 = time.perf_counter()
            n = npres = 0
            for rb in r.raw_blocks():
                n += len(rb["skip"]); npres += int(rb["n_present"].sum())
            dt = time.perf_counter() - t0
            st = r.stats()
            r.close()
        assert n == meta["records"], (n, meta["records"])
        print(json.dumps(dict(base, reader=("native, sample columns on the device" if eng else "native reader, host tokeniser (host pool)"), seconds=dt,
                              records_per_s=n / dt, text_GB_per_s=meta["text_bytes"] / 1e9 / dt, sample_bytes=st["sample_bytes"], launches=st["launches"],
                              present_calls=npres, block=o.block)))
        if eng is not None:
            eng.close()


if __name__ == "__main__":
    main()
