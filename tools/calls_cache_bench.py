"""The per-variant command line from a call cache (--load-calls) against the text it was written from, and k_calls_select alone.

  python tools/calls_cache_bench.py --dir /tmp/callscache > profiles/r21/calls_cache.txt

Input: N = 5000 phenotyped samples among 5200 columns of a VCF in BGZF, 2000 distinct records tiled to --records; every second record carries
missing calls (6 % of its calls), --max-missing 0.1 keeps those rows inside the filters (the records of tools/calls_job_bench.py).  Two caches are
written from it: one by a run with --save-calls over the 5000 (the run's own list), one by pyseer_amd.pack over all 5200 columns (a superset,
in the file's order: the run's 5000 are a random subset in random order).  Runs: `python -m pyseer_amd` called in process, stdout to /dev/null,
fixed effects with ten structure components (--load-m) and --lmm (--load-lmm), as tools/calls_job_bench.py sets them up.  Per model the four
routes alternate in one session -- the text with --device-calls, the same-list cache, the superset cache through the fused submit
(sh_job_submit_calls_select), the superset cache with SEERHIP_ROUTE=calls_cache=rows (sh_select_calls to the host, then sh_job_submit_calls) --
one warm-up run each, then --passes timed runs each: the median of the block loop's rows/s (`[cli budget]` wall_s) with the spread.
k_calls_select alone: one block of 16 384 rows (a block of the route) and one of 262 144 on the device through RowSelector.select_calls_dev, the time
between stream events around the launch, and the bytes of rows it moves (both planes read at the source width and written at the run's; the map is 4 N bytes per group of rows).
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_PHENO, N_COLS, DISTINCT = 5000, 5200, 2000


def make_inputs(d, records):
    """gen.vcf.gz, pheno.tsv, all.txt (the 5200 columns in file order), proj.pkl, lmm.npz under d -> dict of paths"""
    import numpy as np
    import pandas as pd
    from _vcf_text import bgzf_bytes
    os.makedirs(d, exist_ok=True)
    meta = os.path.join(d, "meta.json")
    want = {"records": records, "version": 1}
    paths = {k: os.path.join(d, k) for k in ("gen.vcf.gz", "pheno.tsv", "all.txt", "proj.pkl", "lmm.npz")}
    if os.path.exists(meta) and json.load(open(meta)) == want and all(os.path.exists(p) for p in paths.values()):
        return paths
    rng = np.random.default_rng(7)
    cols = ["s%d" % i for i in rng.permutation(N_COLS)]
    pheno = ["s%d" % i for i in rng.permutation(N_COLS)[:N_PHENO]]
    tok = np.array(["0", "1", "."], dtype=object)
    head = "##fileformat=VCFv4.2\n##contig=<ID=chr1>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" \
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(cols) + "\n"
    vcf = []
    for r in range(DISTINCT):
        af = rng.uniform(0.02, 0.98)
        miss = 0.06 if r % 2 else 0.0
        calls = tok[rng.choice(3, size=N_COLS, p=[(1 - af) * (1 - miss), af * (1 - miss), miss])]
        vcf.append("chr1\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t" % (r + 1) + "\t".join(calls) + "\n")
    with open(paths["gen.vcf.gz"], "wb") as f:
        f.write(bgzf_bytes(head.encode(), level=1)[:-28])
        comp = bgzf_bytes("".join(vcf).encode(), level=1)[:-28]
        for _ in range((records + DISTINCT - 1) // DISTINCT):
            f.write(comp)
        f.write(bgzf_bytes(b"")[-28:])
    y = (rng.random(N_PHENO) < 0.5).astype(int)
    with open(paths["pheno.tsv"], "w") as f:
        f.write("samples\tbinary\n" + "".join("%s\t%d\n" % (s, v) for s, v in zip(pheno, y)))
    with open(paths["all.txt"], "w") as f:
        f.write("".join(s + "\n" for s in cols))
    pd.DataFrame(rng.standard_normal((N_PHENO, 10)), index=pheno).to_pickle(paths["proj.pkl"])
    U, _ = np.linalg.qr(rng.standard_normal((N_PHENO, N_PHENO)))
    np.savez(paths["lmm.npz"], U, np.sort(rng.uniform(0.05, 4.0, N_PHENO))[::-1].copy(), np.array([0.5]))
    json.dump(want, open(meta, "w"))
    return paths


def kernel(n_rows=16384, passes=3):
    """k_calls_select alone: n_rows rows of both planes over 5200 samples -> a random 5000 in random order, on the device"""
    import numpy as np
    import torch
    from pyseer_amd.engine import Engine, RowSelector
    from pyseer_amd.packing import row_bytes_for
    rng = np.random.default_rng(3)
    m = rng.permutation(N_COLS)[:N_PHENO].astype(np.int32)
    e = Engine(N_PHENO)
    sel = RowSelector(e, N_COLS, m)
    src_rb, out_rb = row_bytes_for(N_COLS), row_bytes_for(N_PHENO)
    present = torch.from_numpy(rng.integers(0, 256, (n_rows, src_rb), dtype=np.uint8)).cuda()
    missing = torch.from_numpy((rng.integers(0, 256, (n_rows, src_rb), dtype=np.uint8) & rng.integers(0, 256, (n_rows, src_rb), dtype=np.uint8))
                               * (np.arange(n_rows) % 2 == 1)[:, None].astype(np.uint8)).cuda()
    t = []
    for it in range(passes + 1):
        sel.select_calls_dev(present, missing)
        if it:
            t.append(sel.kernel_seconds())
    sel.close(); e.close()
    moved = 2 * n_rows * (src_rb + out_rb) + 8 * n_rows
    med = statistics.median(t)
    print(json.dumps({"what": "k_calls_select alone (stream events)", "rows_in_block": n_rows, "n_src": N_COLS, "n_dst": N_PHENO, "seconds_median": med,
                      "seconds_min": min(t), "seconds_max": max(t), "rows_per_s": n_rows / med, "row_bytes_moved": moved, "GB_per_s_of_rows": moved / med * 1e-9,
                      "map_bytes_loaded_per_group_of_4_rows": 4 * N_PHENO}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/callscache")
    ap.add_argument("--records", type=int, default=200000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--models", default="fixed,lmm")
    ap.add_argument("--skip-kernel", action="store_true")
    o = ap.parse_args()
    from calls_job_bench import run_cli
    from pyseer_amd import pack
    os.environ["SEERHIP_DEBUG"] = "cli"
    os.environ.pop("SEERHIP_ROUTE", None)
    t0 = time.perf_counter()
    paths = make_inputs(o.dir, o.records)
    print(json.dumps({"what": "inputs", "records": o.records, "seconds_to_make": time.perf_counter() - t0}), flush=True)
    own, sup = os.path.join(o.dir, "own.seercalls"), os.path.join(o.dir, "all.seercalls")
    base = ["--phenotypes", paths["pheno.tsv"], "--max-missing", "0.1"]
    t0 = time.perf_counter()
    r = run_cli(["--vcf", paths["gen.vcf.gz"], "--load-m", paths["proj.pkl"], "--device-calls", "--save-calls", own] + base)
    t1 = time.perf_counter()
    err = sys.stderr
    sys.stderr = open(os.devnull, "w")
    try:
        pack.main([paths["all.txt"], "--vcf", paths["gen.vcf.gz"], "-o", sup])
    finally:
        sys.stderr.close()
        sys.stderr = err
    print(json.dumps({"what": "caches written", "rows": r["rows"], "save_calls_run_loop_s": r["loop_s"], "save_calls_run_s": t1 - t0, "pack_s": time.perf_counter() - t1,
                      "same_list_cache_bytes": os.path.getsize(own), "superset_cache_bytes": os.path.getsize(sup), "text_bytes": os.path.getsize(paths["gen.vcf.gz"])}),
          flush=True)
    routes = {"text --device-calls": (["--vcf", paths["gen.vcf.gz"], "--device-calls"], None),
              "same-list cache": (["--load-calls", own], None),
              "superset cache, fused submit": (["--load-calls", sup], None),
              "superset cache, calls_cache=rows": (["--load-calls", sup], "calls_cache=rows")}
    for model in o.models.split(","):
        tail = base + (["--load-m", paths["proj.pkl"]] if model == "fixed" else ["--lmm", "--load-lmm", paths["lmm.npz"]])
        runs = {k: [] for k in routes}
        for it in range(o.passes + 1):
            for k, (argv, route) in routes.items():              # alternately, in one session; pass 0 warms up
                if route:
                    os.environ["SEERHIP_ROUTE"] = route
                try:
                    r = run_cli(argv + tail)
                finally:
                    os.environ.pop("SEERHIP_ROUTE", None)
                assert r["job_path"]
                if it:
                    runs[k].append(r)
        res = {"what": "command line", "model": model}
        for k, rr in runs.items():
            rate = [x["rows"] / x["loop_s"] for x in rr]
            res[k] = {"rows": rr[0]["rows"], "rows_per_s_median": statistics.median(rate), "rows_per_s_min": min(rate), "rows_per_s_max": max(rate),
                      "loop_s": [x["loop_s"] for x in rr], "waited_for_reader_s": [x["reader_wait_s"] for x in rr]}
        for k in list(routes)[1:]:
            res["ratio to the text: " + k] = res[k]["rows_per_s_median"] / res["text --device-calls"]["rows_per_s_median"]
        print(json.dumps(res), flush=True)
    if not o.skip_kernel:
        kernel(16384)                                            # a block of the route
        kernel(262144)                                           # a launch long enough to show the kernel's own rate


if __name__ == "__main__":
    main()
