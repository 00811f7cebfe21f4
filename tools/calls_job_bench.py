"""The per-variant command line on --vcf (text BGZF, BCF) and --pres with and without --device-calls, on one generated call set.

  python tools/calls_job_bench.py --dir /tmp/callsbench > profiles/r20/calls_job.txt

Input: N = 5000 phenotyped samples among 5200 columns, 2000 distinct records tiled to --records; half of the records carry missing calls (6 % of
their calls: ~3 % of all calls), the others none.  The same records as VCF text in BGZF, as BCF (tests/_bcf_bytes.py) and as an Rtab, written
with the writers tools/bench_vcf_reader.py and tools/bench_rtab_reader.py use.  Runs: `python -m pyseer_amd` called in process (main(argv)), fixed
effects with ten structure components (a projection made here and read with --load-m: the MDS of a 5000 x 5000 distance matrix is set-up time, not
the route's) and --lmm (a cache made here, --load-lmm), --max-missing 0.1 so that the rows with missing calls stay inside the filters, stdout to
/dev/null.  Per model and format the two routes alternate: one warm-up run each, then --passes timed runs each; the median of the block loop's
rows/s (SEERHIP_DEBUG=cli, `[cli timing]`: the time from the first block asked for to the last row written -- set-up excluded) with the spread.
The default route reads the first --slow-records records of the same file (its per-variant Python makes a full pass minutes long); it is the code
of the route before --device-calls existed.  Also printed: the job stream's wait for the reader against its loop time, and the two new kernels'
own times from stream events around them (Job.set_calls_timing).  Prints one JSON line per measurement."""
import argparse
import io
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_inputs(d, records, slow_records):
    """gen.vcf.gz / gen.bcf / gen.Rtab (and their first slow_records records as slow.*), pheno.tsv, proj.pkl, lmm.npz under d -> dict of paths"""
    import struct
    import numpy as np
    import pandas as pd
    from _bcf_bytes import bcf_from_vcf_text
    from _vcf_text import bgzf_bytes
    os.makedirs(d, exist_ok=True)
    meta = os.path.join(d, "meta.json")
    want = {"records": records, "slow": slow_records, "version": 1}
    paths = {k: os.path.join(d, k) for k in ("gen.vcf.gz", "gen.bcf", "gen.Rtab", "slow.vcf.gz", "slow.bcf", "slow.Rtab", "pheno.tsv", "proj.pkl", "lmm.npz")}
    if os.path.exists(meta) and json.load(open(meta)) == want and all(os.path.exists(p) for p in paths.values()):
        return paths
    rng = np.random.default_rng(7)
    n_pheno, n_cols, distinct = 5000, 5200, 2000
    cols = ["s%d" % i for i in rng.permutation(n_cols)]
    pheno = ["s%d" % i for i in rng.permutation(n_cols)[:n_pheno]]
    tok = np.array(["0", "1", "."], dtype=object)
    head = "##fileformat=VCFv4.2\n##contig=<ID=chr1>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" \
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(cols) + "\n"
    vcf, rtab = [], []
    for r in range(distinct):
        af = rng.uniform(0.02, 0.98)
        miss = 0.06 if r % 2 else 0.0
        calls = tok[rng.choice(3, size=n_cols, p=[(1 - af) * (1 - miss), af * (1 - miss), miss])]
        vcf.append("chr1\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t" % (r + 1) + "\t".join(calls) + "\n")
        rtab.append("chr1_%d_A_C\t" % (r + 1) + "\t".join(calls) + "\n")
    body = "".join(vcf).encode()

    def tiled(n):
        return (n + distinct - 1) // distinct
    for name, n in (("gen", records), ("slow", slow_records)):
        with open(paths[name + ".vcf.gz"], "wb") as f:
            f.write(bgzf_bytes(head.encode(), level=1)[:-28])
            comp = bgzf_bytes(body, level=1)[:-28]
            for _ in range(tiled(n)):
                f.write(comp)
            f.write(bgzf_bytes(b"")[-28:])
        raw = bcf_from_vcf_text(head.encode() + body, container=False)
        head_end = 9 + struct.unpack("<I", raw[5:9])[0]
        with open(paths[name + ".bcf"], "wb") as f:
            f.write(bgzf_bytes(raw[:head_end], level=1)[:-28])
            comp = bgzf_bytes(raw[head_end:], level=1)[:-28]
            for _ in range(tiled(n)):
                f.write(comp)
            f.write(bgzf_bytes(b"")[-28:])
        with open(paths[name + ".Rtab"], "w") as f:
            f.write("Gene\t" + "\t".join(cols) + "\n")
            for _ in range(tiled(n)):
                f.write("".join(rtab))
    y = (rng.random(n_pheno) < 0.5).astype(int)
    with open(paths["pheno.tsv"], "w") as f:
        f.write("samples\tbinary\n" + "".join("%s\t%d\n" % (s, v) for s, v in zip(pheno, y)))
    pd.DataFrame(rng.standard_normal((n_pheno, 10)), index=pheno).to_pickle(paths["proj.pkl"])
    U, _ = np.linalg.qr(rng.standard_normal((n_pheno, n_pheno)))
    np.savez(paths["lmm.npz"], U, np.sort(rng.uniform(0.05, 4.0, n_pheno))[::-1].copy(), np.array([0.5]))
    json.dump(want, open(meta, "w"))
    return paths


def run_cli(argv):
    """main(argv) with stdout to /dev/null -> the `[cli timing] stream 0` facts: rows, loop seconds, seconds waited for the reader (job stream only)"""
    from pyseer_amd.__main__ import main
    out, err = sys.stdout, sys.stderr
    sys.stdout, sys.stderr = open(os.devnull, "w"), io.StringIO()
    try:
        main(argv)
        text = sys.stderr.getvalue()
    finally:
        sys.stdout.close()
        sys.stdout, sys.stderr = out, err
    m = re.search(r"\[cli timing\] stream 0 of 1[^:]*: \d+ blocks, (\d+) rows in ([0-9.]+) s of the block loop", text)
    w = re.search(r"this thread waited ([0-9.]+) s for the reader", text)
    budget = json.loads(re.search(r"\[cli budget\] (\{.*\})", text).group(1))
    return {"rows": int(m.group(1)), "loop_s": budget["wall_s"], "reader_wait_s": float(w.group(1)), "job_path": budget["job_path"]}


def kernels(n_rows=16384, passes=3):
    """k_job_calls_mark and k_job_md5_calls alone, from stream events around them (Job.set_calls_timing): blocks of n_rows rows at N = 5000, half
    of the rows with 6 % missing calls, through a fixed-effects job that counts patterns; one warm-up block, then `passes` timed ones."""
    import numpy as np
    from pyseer_amd.engine import Engine, Job, PatternSet, pack_variants
    from pyseer_amd.model import fit_null
    N = 5000
    rng = np.random.default_rng(3)
    y = (rng.random(N) < 0.5).astype(float)
    W = rng.standard_normal((N, 3))
    e = Engine(N)
    e.set_af_filter(0.01, 0.99)
    e0 = np.zeros((0, 0))
    e.glm_setup(y, W, False, fit_null(y, W, e0, False).llf, fit_null(y, W, e0, False, firth=True), 1.0, 1.0)
    af = rng.uniform(0.02, 0.98, n_rows)
    P = (rng.random((n_rows, N)) < af[:, None]).astype(np.uint8)
    M = ((rng.random((n_rows, N)) < 0.06) & (np.arange(n_rows) % 2 == 1)[:, None]).astype(np.uint8)
    P[M == 1] = 0
    pp, mp = pack_variants(P), pack_variants(M)
    n_p, n_m = P.sum(axis=1).astype(np.int32), M.sum(axis=1).astype(np.int32)
    names = b"".join(b"r%07d" % i for i in range(n_rows)); off = np.arange(n_rows + 1, dtype=np.int64) * 8
    skip = np.zeros(n_rows, np.int32)
    ps = PatternSet(e)
    job = Job(e, False, pattern_count=True)
    job.set_calls_timing(True)
    res = []
    for it in range(passes + 1):
        job.submit_calls(pp, mp, n_p, n_m, skip, names, off, 0.1)
        job.collect()
        res.append(job.calls_times())
    job.close(); ps.close(); e.close()
    plane = pp.nbytes
    for kname, rows, nbytes in (("k_job_calls_mark", n_rows, 2 * plane // 2 + 12 * n_rows), ("k_job_md5_calls", n_rows // 2, 2 * plane // 2)):
        t = [r[kname][0] for r in res[1:]]
        print(json.dumps({"what": kname + " alone (stream events)", "rows_in_block": n_rows, "rows_with_missing_calls": n_rows // 2, "N": N,
                          "seconds_median": statistics.median(t), "seconds_min": min(t), "seconds_max": max(t), "launches_per_pass": res[1][kname][1],
                          "rows_it_works_on_per_s": rows / statistics.median(t), "bytes_of_planes_it_reads": nbytes}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/callsbench")
    ap.add_argument("--records", type=int, default=40000)
    ap.add_argument("--slow-records", type=int, default=2000, help="records of the prefix the default route is timed on")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--formats", default="vcf.gz,bcf,Rtab")
    ap.add_argument("--models", default="fixed,lmm")
    ap.add_argument("--skip-kernels", action="store_true")
    o = ap.parse_args()
    os.environ["SEERHIP_DEBUG"] = "cli"
    t0 = time.perf_counter()
    paths = make_inputs(o.dir, o.records, o.slow_records)
    print(json.dumps({"what": "inputs", "records": o.records, "default_route_prefix": o.slow_records, "seconds_to_make": time.perf_counter() - t0}), flush=True)
    for model in o.models.split(","):
        tail = ["--phenotypes", paths["pheno.tsv"], "--max-missing", "0.1"] + \
               (["--load-m", paths["proj.pkl"]] if model == "fixed" else ["--lmm", "--load-lmm", paths["lmm.npz"]])
        for fmt in o.formats.split(","):
            flag = "--pres" if fmt == "Rtab" else "--vcf"
            routes = {"default": [flag, paths["slow." + fmt]] + tail, "device-calls": [flag, paths["gen." + fmt]] + tail + ["--device-calls"]}
            runs = {k: [] for k in routes}
            for it in range(o.passes + 1):
                for k, argv in routes.items():                      # alternately, in one session; pass 0 warms up
                    r = run_cli(argv)
                    assert r["job_path"] == (k == "device-calls")
                    if it:
                        runs[k].append(r)
            res = {"what": "command line", "model": model, "format": fmt}
            for k, rr in runs.items():
                rate = [x["rows"] / x["loop_s"] for x in rr]
                res[k] = {"rows": rr[0]["rows"], "rows_per_s_median": statistics.median(rate), "rows_per_s_min": min(rate), "rows_per_s_max": max(rate),
                          "loop_s": [x["loop_s"] for x in rr], "waited_for_reader_s": [x["reader_wait_s"] for x in rr]}
            res["ratio"] = res["device-calls"]["rows_per_s_median"] / res["default"]["rows_per_s_median"]
            print(json.dumps(res), flush=True)
    if not o.skip_kernels:
        kernels()


if __name__ == "__main__":
    main()
