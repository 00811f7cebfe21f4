"""Rates of the Rtab readers on a generated presence/absence table: N = 5000 phenotyped samples among 5200 shuffled columns, ~3 % missing calls
(half `.`, half empty), 2000 distinct rows tiled to --rows.

  python tools/bench_rtab_reader.py --dir /tmp/rtabbench                               # (a) native end to end, (b) host tokeniser, (c) Python reader
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_rtab_reader.py --dir /tmp/rtabbench --only native --passes 1
  python tools/bench_rtab_reader.py --kernel-stats OUT --traced-json <the traced run's output>      # (d) k_rtab_pack alone, from that trace

(a) runs with one wavefront and with one workgroup per line (SEERHIP_ROUTE rtab_wg=64 / 256); (a) and (b) take one warm-up pass over the file (the
page cache, the pinned slabs, the kernel's code object), then --passes timed passes each, the variants alternating, and report every pass and
the median; (c) reads the first --python-rows rows.  (b) is the same reader with the kernel's work done by shrtab::host_rtab_pack on the host
pool.  (d) is the kernel's time on text that is resident in device memory, as the profiler saw it.  Prints one JSON line per measurement."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12          # bytes/s: float4 copy measured, and the specification


def make_file(d, rows):
    """gen.Rtab of `rows` rows and meta.json under d; (path, meta)."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    path, meta = os.path.join(d, "gen.Rtab"), os.path.join(d, "meta.json")
    if os.path.exists(path) and os.path.exists(meta) and json.load(open(meta))["rows"] == rows:
        return path, json.load(open(meta))
    rng = np.random.default_rng(7)
    n_pheno, n_cols, distinct = 5000, 5200, 2000
    cols = ["s%d" % i for i in rng.permutation(n_cols)]
    pheno = ["s%d" % i for i in rng.permutation(n_pheno)]
    tokens = np.array(["0", "1", ".", ""], dtype=object)
    body = []
    for r in range(distinct):
        af = rng.uniform(0.02, 0.98)
        calls = tokens[rng.choice(4, size=n_cols, p=[(1 - af) * 0.97, af * 0.97, 0.015, 0.015])]
        if calls[-1] == "":
            calls[-1] = "0"
        body.append(("unitig_%06d\t" % r + "\t".join(calls) + "\n").encode())
    body = b"".join(body)
    head = ("Gene\t" + "\t".join(cols) + "\n").encode()
    tiles = -(-rows // distinct)
    with open(path, "wb") as f:
        f.write(head)
        for _ in range(tiles):
            f.write(body)
    m = {"rows": rows, "file_rows": distinct * tiles, "text_bytes": len(head) + tiles * len(body), "samples": pheno, "columns": n_cols}
    json.dump(m, open(meta, "w"))
    return path, m


def kernel_stats(out_dir):
    rows = []
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    out = [{"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]), "total_s": float(r["TotalDurationNs"]) * 1e-9, "mean_us": float(r["AverageNs"]) * 1e-3}
           for r in rows if "k_rtab_pack" in r["Name"]]
    if not out:
        raise SystemExit("no k_rtab_pack row under " + out_dir)
    return out


def one_pass(path, samples, eng, block):
    from pyseer_amd.input import NativeRtabReader
    r = NativeRtabReader(path, samples, eng, block)
    t0 = time.perf_counter()
    n = npres = 0
    for rb in r.raw_blocks():                              # (every block ends in a stream synchronise inside sh_rtab_next)
        n += len(rb["status"]); npres += int(rb["n_present"].sum())
    dt = time.perf_counter() - t0
    st = r.stats()
    r.close()
    return dt, n, npres, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/rtabbench")
    ap.add_argument("--rows", type=int, default=40000)
    ap.add_argument("--only", default=None, choices=["python", "native", "host"])
    ap.add_argument("--python-rows", type=int, default=2000)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--block", type=int, default=3000)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--traced-json", default=None, help="with --kernel-stats: the JSON lines the traced run printed (call bytes and rows of a pass per launch shape)")
    o = ap.parse_args()
    if o.kernel_stats:
        traced = {}
        if o.traced_json:
            for line in open(o.traced_json).read().splitlines():
                if line.startswith("{") and "wg" in json.loads(line):
                    traced[json.loads(line)["wg"]] = json.loads(line)
        for k in kernel_stats(o.kernel_stats):
            wg = int(k["kernel"].split("<")[1].split(">")[0].split(",")[0]) if "<" in k["kernel"] else None
            if wg in traced:
                t = traced[wg]
                passes = 1 + len(t["seconds_per_pass"])                      # the warm-up pass ran the kernel too
                k["rows"], k["call_bytes"] = passes * t["rows"], passes * t["call_bytes"]
                k["rows_per_s"], k["bytes_per_s"] = k["rows"] / k["total_s"], k["call_bytes"] / k["total_s"]
                k["share_of_measured_hbm_copy_rate"], k["share_of_hbm_spec"] = k["bytes_per_s"] / HBM_MEASURED, k["bytes_per_s"] / HBM_SPEC
            print(json.dumps(k))
        return
    path, meta = make_file(o.dir, o.rows)
    samples = meta["samples"]
    base = {"rows": meta["file_rows"], "text_GB": meta["text_bytes"] / 1e9, "n_samples": len(samples), "columns": meta["columns"]}
    if o.only in (None, "python"):
        import contextlib
        import io
        import pandas as pd
        from pyseer_amd.input import open_variant_file, read_variant
        p = pd.Series(0.0, index=samples)
        infile, order = open_variant_file("Rtab", path)
        strains = set(p.index)
        t0 = time.perf_counter()
        n = 0
        with contextlib.redirect_stderr(io.StringIO()):
            while n < o.python_rows and not read_variant(infile, p, "Rtab", False, None, False, strains, order)[0]:
                n += 1
        dt = time.perf_counter() - t0
        print(json.dumps(dict(base, reader="python (read_variant, first %d rows)" % n, seconds=dt, rows_per_s=n / dt)), flush=True)
    variants = []
    if o.only in (None, "native"):
        from pyseer_amd.engine import Engine
        eng = Engine(len(samples))
        variants += [("native, calls on the device, one wavefront per line", eng, 64), ("native, calls on the device, one workgroup per line", eng, 256)]
    if o.only in (None, "host"):
        variants.append(("native reader, host tokeniser (host pool)", None, None))
    times = {v[0]: [] for v in variants}
    last = {}
    for rep in range(1 + o.passes):                        # pass 0 warms up; the variants alternate
        for label, eng, wg in variants:
            if wg is not None:
                os.environ["SEERHIP_ROUTE"] = "rtab_wg=%d" % wg
            dt, n, npres, st = one_pass(path, samples, eng, o.block)
            os.environ.pop("SEERHIP_ROUTE", None)
            assert n == meta["file_rows"], (n, meta["file_rows"])
            if rep:
                times[label].append(dt)
            last[label] = (npres, st)
    for label, eng, wg in variants:
        ts = sorted(times[label])
        med = ts[len(ts) // 2]
        npres, st = last[label]
        print(json.dumps(dict(base, reader=label, wg=wg, seconds_per_pass=times[label], median_seconds=med, rows_per_s=meta["file_rows"] / med,
                              text_GB_per_s=meta["text_bytes"] / 1e9 / med, call_bytes=st["call_bytes"], launches=st["launches"], present_calls=npres,
                              block=o.block)), flush=True)
    for _, eng, _ in variants[:1]:
        if eng is not None:
            eng.close()


if __name__ == "__main__":
    main()
