"""What the kinship matrix costs from a packed cache (pyseer_amd/similarity.py main_packed; sh_sim_accumulate_select, sh_sim_text).

A synthetic cache over n_src = 5200 samples, a run over N = 5000 of them in another order, ROWS rows (2^20 unless the environment says
otherwise; profiles/r19/similarity_cache.txt: ROWS=4194304), stored in blocks of 2^18 rows.  Medians of 3 passes after a warm-up pass,
with the passes, all in one process and one session:
  a. the cache's rows (views of its mapping) through sh_sim_accumulate_select: one upload, selected and accumulated on the device;
  b. the same rows through sh_select_rows to the host and then sh_sim_accumulate: the route without that call (three PCIe crossings);
  c. a 5000-sample cache of the same rows over the run's own list through sh_sim_accumulate;
  d. the native text reader on gzip text of the first TEXT_ROWS of the same rows over the run's samples (parsing only), and the
     time that rate gives for ROWS rows: a prefix, scaled;
  e. sh_sim_text alone on the accumulated matrix (the length query, the text, its copy to the host);
  f. pandas.DataFrame.to_csv of the same matrix into memory, on this machine's CPU.
The matrices of a, b and c are compared, and the bytes of e and f.
Usage: python tools/similarity_cache_bench.py [--out FILE]   (ROWS, TEXT_ROWS, TMP from the environment)"""
import io
import os
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pandas as pd                                                    # noqa: E402
from pyseer_amd import _abi                                            # noqa: E402
from pyseer_amd.engine import Engine, RowSelector                      # noqa: E402
from pyseer_amd.input import NativeKmerReader, PackedCacheWriter, open_packed_cache_rows    # noqa: E402
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


def passes(ts, fmt="%.3f"):
    return "passes " + " ".join(fmt % x for x in ts) + ", spread %.0f %%" % (100.0 * (max(ts) - min(ts)) / np.median(ts))


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    tmp = tempfile.mkdtemp(prefix="similarity_cache_", dir=os.environ.get("TMP"))
    rng = np.random.default_rng(0)
    src_rb, dst_rb = row_bytes_for(N_SRC), row_bytes_for(N_DST)
    bits = rng.integers(0, 256, size=(ROWS, src_rb), dtype=np.uint8)   # every sample a carrier of half the rows; the pad bits are noise
    names_src = ["sample_%05d" % i for i in range(N_SRC)]
    sample_map = rng.permutation(N_SRC)[:N_DST].astype(np.int32)
    names_dst = [names_src[i] for i in sample_map]
    say("similarity_cache_bench: n_src %d -> N %d (a random subset in random order), %d rows of %d -> %d bytes in stored blocks of %d; host CPUs %d; "
        "medians of %d passes after a warm-up" % (N_SRC, N_DST, ROWS, src_rb, dst_rb, BLOCK, _abi.load().sh_host_cpus(), PASSES))
    eng = Engine(N_DST)
    eng.set_af_filter(0.01, 0.99)
    sel = RowSelector(eng, N_SRC, sample_map)
    # the two caches: the same rows over 5200 samples and over the run's own 5000
    sel_bits = np.concatenate([sel.select(bits[i:i + BLOCK])[0] for i in range(0, ROWS, BLOCK)])
    blob = b"".join(b"K%07d" % v for v in range(ROWS))
    off = np.arange(ROWS + 1, dtype=np.int64) * 8
    big, own = os.path.join(tmp, "all.seerpack"), os.path.join(tmp, "own.seerpack")
    for path, names, rows in ((big, names_src, bits), (own, names_dst, sel_bits)):
        w = PackedCacheWriter(path, names)
        for i in range(0, ROWS, BLOCK):
            j = min(ROWS, i + BLOCK)
            w.write_block(blob[8 * i:8 * j], off[i:j + 1] - off[i], np.ones(j - i, dtype=np.int32), rows[i:j])
        w.close()
    del sel_bits
    Ks = {}

    def cache_pass(path, feed, key):
        def go():
            _, _, total, rows = open_packed_cache_rows(path)
            assert total == ROWS
            eng.sim_begin()
            for b, _ in rows():
                feed(b)
            eng.synchronize()
        t, ts = median_of(go)
        Ks[key] = eng.sim_finish()
        return t, ts
    t_a, ts = cache_pass(big, sel.sim_accumulate, "a")
    say("a. 5200-sample cache through sh_sim_accumulate_select (one upload, select + accumulate on the device): %.3f s = %.1f M rows/s  (%s)"
        % (t_a, ROWS / t_a / 1e6, passes(ts)))
    t_b, ts = cache_pass(big, lambda b: eng.sim_accumulate(sel.select(b)[0]), "b")
    say("b. the same cache through sh_select_rows to the host, then sh_sim_accumulate: %.3f s = %.1f M rows/s  (%s)" % (t_b, ROWS / t_b / 1e6, passes(ts)))
    t_c, ts = cache_pass(own, eng.sim_accumulate, "c")
    say("c. 5000-sample cache over the run's own list through sh_sim_accumulate: %.3f s = %.1f M rows/s  (%s)" % (t_c, ROWS / t_c / 1e6, passes(ts)))
    assert np.array_equal(Ks["a"], Ks["b"]) and np.array_equal(Ks["a"], Ks["c"])
    say("   the three matrices are equal; largest count %d" % int(Ks["a"].max()))
    # d. gzip text of the first TEXT_ROWS rows, read over the run's 5000 samples
    tok = np.array([n + ":1" for n in names_src], dtype=object)
    dense = np.unpackbits(bits[:TEXT_ROWS], axis=1, bitorder="little")[:, :N_SRC].astype(bool)
    gz = os.path.join(tmp, "k.gz")
    co = zlib.compressobj(1, zlib.DEFLATED, 31)
    with open(gz, "wb") as f:
        for v0 in range(0, TEXT_ROWS, 512):
            f.write(co.compress("".join("K%07d | %s\n" % (v, " ".join(tok[dense[v]])) for v in range(v0, min(TEXT_ROWS, v0 + 512))).encode()))
        f.write(co.flush())
    del dense

    def read_text():
        r = NativeKmerReader(gz, names_dst, 4096)
        n = 0
        for b, counts, _, _ in r.raw_blocks():
            n += counts.shape[0]
        r.close()
        assert n == TEXT_ROWS
    t_d, ts = median_of(read_text)
    say("d. native text reader, gzip text of the first %d rows over the run's 5000 samples: %.3f s = %.3f M rows/s  (%s); scaled to %d rows: %.0f s, "
        "%.0f x the time of a" % (TEXT_ROWS, t_d, TEXT_ROWS / t_d / 1e6, passes(ts), ROWS, t_d * ROWS / TEXT_ROWS, (t_d * ROWS / TEXT_ROWS) / t_a))
    # e, f: the matrix as text (the accumulator still holds c's matrix)
    got = [None]

    def dev_text():
        got[0] = eng.sim_text(names_dst)
    t_e, ts = median_of(dev_text)
    say("e. sh_sim_text of the %d x %d matrix (length query + text + copy to the host): %.3f s for %.1f MB = %.2f GB/s  (%s)"
        % (N_DST, N_DST, t_e, got[0].shape[0] / 1e6, got[0].shape[0] / t_e / 1e9, passes(ts)))
    ref = [None]

    def host_text():
        s = io.StringIO()
        pd.DataFrame(Ks["c"], index=names_dst, columns=names_dst).to_csv(s, sep='\t')
        ref[0] = s.getvalue()
    t_f, ts = median_of(host_text)
    say("f. pandas to_csv of the same matrix into memory: %.2f s  (%s); %.0f x the time of e; the bytes are equal: %s"
        % (t_f, passes(ts, "%.2f"), t_f / t_e, ref[0].encode() == got[0].tobytes()))
    sel.close(); eng.close()
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines_out) + "\n")


if __name__ == "__main__":
    main()
