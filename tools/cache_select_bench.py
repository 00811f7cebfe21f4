"""What serving a packed cache to a subset of its samples costs (pyseer_amd/input.py iter_packed_blocks_cached, select; k_rows_select).

A synthetic cache over n_src = 5200 samples, a run over N = 5000 of them in another order, ROWS rows (2^20 unless the
environment says otherwise; profiles/r17/cache_select.txt: ROWS=4194304).  Medians of 3 passes after a
warm-up pass, all in one process and one session:
  1. k_rows_select alone (device rows in, device rows out; the host clock around the synchronous sh_select_rows_dev): rows/s and GB/s of
     source + output rows;
  2. sh_select_rows (host rows in and out: the staging copies and two PCIe crossings included);
  3. sh_select_rows_host on the CPUs this process may use;
  4. the iterator end to end (blocks of 2^18 rows handed to a consumer that drops them):
       a. the 5200-sample cache through the select route (device), b. the same through the host restatement,
       c. a 5000-sample cache of the same rows over the run's own list -- the path a cache has always taken (the baseline),
       d. the native text reader on gzip text of the first TEXT_ROWS of the same rows: what the run costs without the feature;
  5. the command line (fixed effects, no covariates) on cache (a) through the select route and on cache (c) with SEERHIP_ROUTE=job=py, the
     same Python block loop: the block loop's own rows/s ([cli timing], SEERHIP_DEBUG=cli).
Usage: python tools/cache_select_bench.py [--out FILE]   (ROWS, TEXT_ROWS, TMP from the environment)"""
import os
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pandas as pd                                                    # noqa: E402
from pyseer_amd import _abi                                            # noqa: E402
from pyseer_amd.engine import Engine, RowSelector, select_rows_host    # noqa: E402
from pyseer_amd.input import NativeKmerReader, PackedCacheWriter, iter_packed_blocks_cached    # noqa: E402
from pyseer_amd.packing import row_bytes_for                           # noqa: E402

N_SRC, N_DST = 5200, 5000
ROWS = int(os.environ.get("ROWS", 1 << 20))
TEXT_ROWS = int(os.environ.get("TEXT_ROWS", 24576))
BLOCK = 1 << 18
PASSES = 3
lines_out = []


def say(s):
    print(s, flush=True)
    lines_out.append(s)


def median_of(fn):
    fn()                                                               # warm-up
    ts = []
    for _ in range(PASSES):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def main():
    import torch
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    tmp = tempfile.mkdtemp(prefix="cache_select_", dir=os.environ.get("TMP"))
    rng = np.random.default_rng(0)
    src_rb, dst_rb = row_bytes_for(N_SRC), row_bytes_for(N_DST)
    bits = rng.integers(0, 256, size=(ROWS, src_rb), dtype=np.uint8)   # every sample a carrier of half the rows; the pad bits are noise
    names_src = ["sample_%05d" % i for i in range(N_SRC)]
    sample_map = rng.permutation(N_SRC)[:N_DST].astype(np.int32)
    names_dst = [names_src[i] for i in sample_map]
    say("cache_select_bench: n_src %d -> N %d (a random subset in random order), %d rows of %d -> %d bytes; host CPUs %d; medians of %d passes after a warm-up"
        % (N_SRC, N_DST, ROWS, src_rb, dst_rb, _abi.load().sh_host_cpus(), PASSES))
    eng = Engine(N_DST)
    sel = RowSelector(eng, N_SRC, sample_map)
    gb = ROWS * (src_rb + dst_rb) / 1e9
    # 1. the kernel alone, in slices of one block
    d_bits = [torch.from_numpy(bits[i:i + BLOCK]).cuda() for i in range(0, ROWS, BLOCK)]
    t, ts = median_of(lambda: [sel.select_dev(b) for b in d_bits])
    say("1. k_rows_select alone (device to device, %d launches of %d rows, outputs allocated inside): %.4f s = %.1f M rows/s, %.1f GB/s of rows read + written  (passes %s)"
        % (len(d_bits), BLOCK, t, ROWS / t / 1e6, gb / t, " ".join("%.4f" % x for x in ts)))
    del d_bits
    torch.cuda.empty_cache()
    # 2. host in, host out
    got = [None]

    def host_inout():
        got[0] = [sel.select(bits[i:i + BLOCK]) for i in range(0, ROWS, BLOCK)]
    t, ts = median_of(host_inout)
    say("2. sh_select_rows (host rows in, host rows out, blocks of %d): %.3f s = %.1f M rows/s  (passes %s)" % (BLOCK, t, ROWS / t / 1e6, " ".join("%.3f" % x for x in ts)))
    sel_bits = np.concatenate([g[0] for g in got[0]]); sel_counts = np.concatenate([g[1] for g in got[0]])
    # 3. the host restatement
    t, ts = median_of(lambda: select_rows_host(bits, N_SRC, sample_map))
    hb, hc = select_rows_host(bits, N_SRC, sample_map)
    assert np.array_equal(hb, sel_bits) and np.array_equal(hc, sel_counts)
    say("3. sh_select_rows_host (the host pool): %.3f s = %.2f M rows/s  (passes %s); its rows and counts equal the device's" % (t, ROWS / t / 1e6, " ".join("%.3f" % x for x in ts)))
    del hb, hc
    # the two caches: the same rows over 5200 and over the run's own 5000 (names K%07d)
    blob = b"".join(b"K%07d" % v for v in range(ROWS))
    off = np.arange(ROWS + 1, dtype=np.int64) * 8
    big, own = os.path.join(tmp, "all.seerpack"), os.path.join(tmp, "own.seerpack")
    for path, names, rows, counts in ((big, names_src, bits, np.zeros(ROWS, dtype=np.int32)), (own, names_dst, sel_bits, sel_counts)):
        w = PackedCacheWriter(path, names)
        for i in range(0, ROWS, BLOCK):
            j = min(ROWS, i + BLOCK)
            w.write_block(blob[8 * i:8 * j], off[i:j + 1] - off[i], counts[i:j], rows[i:j])
        w.close()
    p = pd.Series(np.arange(N_DST) % 2, index=names_dst)

    def walk(path, select):
        def go():
            n = 0
            for blk in iter_packed_blocks_cached(p, path, 0.0, 1.0, BLOCK, raw=True, device=None, say_empty=False, select=select):
                n += len(blk)
            assert n == ROWS
        return median_of(go)
    t_sel, ts = walk(big, eng)
    say("4a. iterator, 5200-sample cache through the select route (device): %.3f s = %.1f M rows/s  (passes %s)" % (t_sel, ROWS / t_sel / 1e6, " ".join("%.3f" % x for x in ts)))
    t, ts = walk(big, "host")
    say("4b. iterator, 5200-sample cache through the host restatement: %.3f s = %.2f M rows/s  (passes %s)" % (t, ROWS / t / 1e6, " ".join("%.3f" % x for x in ts)))
    t, ts = walk(own, None)
    say("4c. iterator, 5000-sample cache over the run's own list (views of the mapping, no row is touched): %.4f s = %.0f M rows/s  (passes %s)"
        % (t, ROWS / t / 1e6, " ".join("%.4f" % x for x in ts)))
    # 4d. gzip text of the first TEXT_ROWS rows, read over the run's 5000 samples
    tok = np.array([n + ":1" for n in names_src], dtype=object)
    dense = np.unpackbits(bits[:TEXT_ROWS], axis=1, bitorder="little")[:, :N_SRC].astype(bool)
    gz = os.path.join(tmp, "k.gz")
    co = zlib.compressobj(1, zlib.DEFLATED, 31)
    text_bytes = 0
    with open(gz, "wb") as f:
        for v0 in range(0, TEXT_ROWS, 512):
            chunk = "".join("K%07d | %s\n" % (v, " ".join(tok[dense[v]])) for v in range(v0, min(TEXT_ROWS, v0 + 512))).encode()
            text_bytes += len(chunk)
            f.write(co.compress(chunk))
        f.write(co.flush())
    del dense

    def read_text():
        r = NativeKmerReader(gz, names_dst, 4096)
        n, c = 0, 0
        for b, counts, _, _ in r.raw_blocks():
            n += counts.shape[0]; c += int(counts.sum())
        r.close()
        assert n == TEXT_ROWS and c == int(sel_counts[:TEXT_ROWS].sum())
    t_txt, ts = median_of(read_text)
    say("4d. native text reader, gzip text of the first %d rows (%.0f MB of text, %.0f MB gzip) over the run's 5000 samples: %.3f s = %.3f M rows/s  (passes %s)"
        % (TEXT_ROWS, text_bytes / 1e6, os.path.getsize(gz) / 1e6, t_txt, TEXT_ROWS / t_txt / 1e6, " ".join("%.3f" % x for x in ts)))
    say("    select route / text reader, rows per second: %.0f x" % ((ROWS / t_sel) / (TEXT_ROWS / t_txt)))
    sel.close(); eng.close()
    # 5. the command line's block loop, the same Python loop both ways
    pheno = os.path.join(tmp, "run.pheno")
    with open(pheno, "w") as f:
        f.write("samples\tbinary\n" + "".join("%s\t%d\n" % (n, i % 2) for i, n in enumerate(names_dst)))
    env = dict(os.environ); env["PYTHONPATH"] = ROOT; env["SEERHIP_DEBUG"] = "cli"
    for label, path, route in (("5a. command line, 5200-sample cache, select route", big, None),
                               ("5b. command line, 5000-sample cache, SEERHIP_ROUTE=job=py (baseline)", own, "job=py")):
        env.pop("SEERHIP_ROUTE", None)
        if route:
            env["SEERHIP_ROUTE"] = route
        rates, waits, loops = [], [], []
        for k in range(PASSES + 1):
            r = subprocess.run([sys.executable, "-m", "pyseer_amd", "--kmers", gz, "--phenotypes", pheno, "--no-distances", "--lrt-pvalue", "1e-3",
                                "--load-packed", path], env=env,
                               stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
            err = r.stderr.decode()
            assert r.returncode == 0, err[-2000:]
            line = [l for l in err.splitlines() if l.startswith("[cli timing] stream 0")][0]
            if k:
                rates.append(float(line.split(" = ")[1].split(" rows/s")[0]))
                waits.append(float(line.split("this thread waited ")[1].split(" s")[0]))
                loops.append(float(line.split(" rows in ")[1].split(" s")[0]))
        say("%s: block loop %.1f M rows/s  (passes %s); of %.2f s in the loop the consumer waited %.2f s for the reader"
            % (label, np.median(rates) / 1e6, " ".join("%.1f" % (x / 1e6) for x in rates), np.median(loops), np.median(waits)))
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines_out) + "\n")


if __name__ == "__main__":
    main()
