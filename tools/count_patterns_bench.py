"""What --count-patterns costs (ISSUE: count distinct presence patterns on the device).  Prints, and the caller keeps as
profiles/r13/count_patterns.txt:

1. the insert alone: N = 5000, blocks of 2^18 packed rows already in device memory through sh_patset_add_rows_dev -- every row distinct, one
   row in eight distinct, every row present from an earlier block -- as rows/s, against the LMM job's 33 M rows/s;
2. end to end over one packed cache of V random k-mers (every row distinct: the set's worst case), `--lmm --load-packed --no-dedup --lrt-pvalue 1e-3`, five passes each, in
   turn: (a) the parent commit with --output-patterns (PARENT=<a built checkout of it>; left out when unset), (b) this tree with
   --count-patterns only, (c) this tree with neither, and (d) the wall time of the reference script's
   `LC_ALL=C sort -u -S 1014M -T /tmp patterns | wc -l` over (a)'s file.  The figure of a pass is its block loop's rows/s ([cli budget]).

    V=8000000 PARENT=/path/to/parent python tools/count_patterns_bench.py"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from pyseer_amd.engine import Engine, PatternSet
from pyseer_amd.input import PackedCacheWriter
from pyseer_amd.packing import row_bytes_for

N = 5000
V = int(os.environ.get("V", 8_000_000))
BLK = 1 << 18
PASSES = int(os.environ.get("PASSES", 5))
PARENT = os.environ.get("PARENT")
d = os.environ.get("BENCH_DIR", "/tmp/count_patterns_bench"); os.makedirs(d, exist_ok=True)
dev = torch.device("cuda", 0)
rb = row_bytes_for(N)
LMM_ROWS_PER_S = 33e6


def spread(xs):
    return "median %.4g, min %.4g, max %.4g" % (statistics.median(xs), min(xs), max(xs))


# ---- 1. the insert alone ---------------------------------------------------------------------------------------------------------------------
def insert_alone():
    e = Engine(N)
    blocks = [bench.synth_bits(BLK, N, rb, 100 + i, dev) for i in range(4)]
    eighth = [b[torch.arange(BLK, device=dev) // 8 * 8].contiguous() for b in blocks]
    torch.cuda.synchronize()
    print("1. the insert alone: N = %d (%d bytes a row), blocks of %d rows in device memory, table of 2^24 slots to begin with" % (N, rb, BLK))
    for name, first, timed in (("every row distinct", [], blocks), ("one row in eight distinct", [], eighth), ("every row already present", blocks, blocks)):
        ps = PatternSet(e, 1 << 24)
        for b in first:
            ps.add_rows_dev(b)
        before = ps.count()
        rates = []
        for b in timed:
            t0 = time.perf_counter()
            ps.add_rows_dev(b)
            n = ps.count()                                         # (waits for the insert)
            rates.append(BLK / (time.perf_counter() - t0))
        d_, slots, growths = ps.info()
        ps.close()
        print("   %-28s %s rows/s = %.0f x the LMM job's 33 M rows/s; %d -> %d distinct, %d slots, %d growths"
              % (name + ":", spread(rates), statistics.median(rates) / LMM_ROWS_PER_S, before, n, slots, growths), flush=True)
    e.close()


# ---- 2. end to end ---------------------------------------------------------------------------------------------------------------------------
def write_inputs():
    names = ["sample_%05d" % i for i in range(N)]
    U, S, h2, C, y, lin = bench.synth_lmm_inputs(N, 1003, dev)
    np.savez(d + "/lmm.npz", U, S, np.array([h2]))
    with open(d + "/pheno.tsv", "w") as f:
        f.write("samples\tbinary\n")
        for i in range(N):
            f.write("%s\t%d\n" % (names[i], int(y[i])))
    open(d + "/kmers.txt", "w").write("AAAA | sample_00000:1\n")
    w = PackedCacheWriter(d + "/kmers.seerpack", names)
    rng = np.random.default_rng(0)
    alphabet = np.frombuffer(b"ACGT", dtype=np.uint8)
    lut = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int32, device=dev)
    for s in range(0, V, BLK):
        nv = min(BLK, V - s)
        bits_t = bench.synth_bits(nv, N, rb, 7000 + s, dev)
        counts = lut[bits_t.long()].sum(dim=1).to(torch.int32).cpu().numpy()
        w.write_block(alphabet[rng.integers(0, 4, 31 * nv)].tobytes(), np.arange(nv + 1, dtype=np.int64) * 31, counts, bits_t.cpu().numpy())
    w.close()
    del U
    torch.cuda.empty_cache()


def one_pass(tree, extra):
    env = dict(os.environ, PYTHONPATH=tree, SEERHIP_DEBUG="cli")
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "pyseer_amd", "--kmers", d + "/kmers.txt", "--uncompressed", "--phenotypes", d + "/pheno.tsv", "--lmm", "--load-lmm",
                        d + "/lmm.npz", "--load-packed", d + "/kmers.seerpack", "--lrt-pvalue", "1e-3", "--no-dedup"] + extra, env=env, cwd=tree,
                       stdout=open(d + "/out.tsv", "w"), stderr=subprocess.PIPE)
    wall = time.time() - t0
    err = r.stderr.decode()
    if r.returncode:
        raise SystemExit("pass failed: " + err[-3000:])
    bl = [l for l in err.splitlines() if l.startswith("[cli budget] ")]
    b = json.loads(bl[-1][len("[cli budget] "):])
    return b["rows"] / b["wall_s"], wall


def end_to_end():
    t0 = time.time()
    write_inputs()
    print("2. end to end: --lmm --load-packed over %d random k-mers x %d samples (every row distinct), cache %.2f GB written in %.0f s; %d passes each, in turn"
          % (V, N, os.path.getsize(d + "/kmers.seerpack") / 1e9, time.time() - t0, PASSES), flush=True)
    runs = [("b", "this tree, --count-patterns only", ROOT, ["--count-patterns", d + "/count.txt"]), ("c", "this tree, neither flag", ROOT, [])]
    if PARENT:
        runs.insert(0, ("a", "the parent commit, --output-patterns", PARENT, ["--output-patterns", d + "/patterns.txt"]))
    one_pass(ROOT, [])                                             # (the cache into the page cache)
    rates = {k: [] for k, _, _, _ in runs}
    for _ in range(PASSES):
        for k, _, tree, extra in runs:
            rates[k].append(one_pass(tree, extra)[0])
            print("      pass (%s): %.4g rows/s" % (k, rates[k][-1]), flush=True)
    for k, what, _, _ in runs:
        print("   (%s) %-40s block loop %s rows/s" % (k, what + ":", spread(rates[k])), flush=True)
    print("   count file: " + open(d + "/count.txt").read().replace("\n", " | ").replace("\t", " "))
    med = {k: statistics.median(v) for k, v in rates.items()}
    print("   (b) / (c) = %.3f" % (med["b"] / med["c"]))
    if PARENT:
        print("   (b) / (a) = %.3f; condition (b) at least as fast as (a) beyond the spread: min(b) %.4g %s max(a) %.4g"
              % (med["b"] / med["a"], min(rates["b"]), ">=" if min(rates["b"]) >= max(rates["a"]) else "<", max(rates["a"])))
        t1 = time.time()
        n = subprocess.check_output("LC_ALL=C sort -u -S 1014M -T /tmp %s | wc -l" % (d + "/patterns.txt"), shell=True, universal_newlines=True).strip()
        print("   (d) sort -u | wc -l over (a)'s pattern file (%.2f GB, the reference script's default options): %.1f s wall, %s distinct lines"
              % (os.path.getsize(d + "/patterns.txt") / 1e9, time.time() - t1, n), flush=True)


if __name__ == "__main__":
    print("device: %s" % torch.cuda.get_device_name(0))
    if os.environ.get("PART", "12").find("1") >= 0:
        insert_alone()
    if os.environ.get("PART", "12").find("2") >= 0:
        end_to_end()
