#!/usr/bin/env python
"""Times prediction from a saved elastic-net model (python -m pyseer_amd.enet_predict) on seeded synthetic input, N = --samples.
One JSON line per measurement: a warm-up, then --repeats timed runs (median, min, max).  Every timed call ends with the device idle
(sh_predict_add synchronises its stream before it returns; whole runs are processes), so no clock is read over queued work.

    python tools/predict_bench.py --stage add          # EnetPredictor.add (gather + upload + k_enet_predict) at S = 1e4, 1e5, 1e6 selected rows
    python tools/predict_bench.py --stage nameset      # sh_nameset_match: names/s over 2^18-name blocks against a model of 1e5 names
    python tools/predict_bench.py --stage cache        # a whole run from a packed cache of 2^20 rows, 1e5 of them in the model
    python tools/predict_bench.py --stage text         # a whole run from gzipped k-mer text, native and --python-reader

The kernel alone is read from a kernel trace of `--stage add --repeats 1` (rocprofv3 --kernel-trace --stats, a run of its own): the
launches of k_enet_predict come in the order of the sizes, ceil(S / rows per upload) each after the warm-up's one."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ts):
    return dict(median_s=float(np.median(ts)), min_s=float(np.min(ts)), max_s=float(np.max(ts)), n=len(ts))


def emit(**kw):
    print(json.dumps(kw), flush=True)


def random_rows(rng, rows, n):
    """Packed rows of about a quarter carriers, padding bits cleared, and their carrier counts."""
    rb = ((n + 63) // 64) * 8
    bits = rng.integers(0, 256, size=(rows, rb), dtype=np.uint8) & rng.integers(0, 256, size=(rows, rb), dtype=np.uint8)
    valid = np.packbits((np.arange(rb * 8) < n).astype(np.uint8), bitorder="little")
    bits &= valid
    pop = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)
    counts = np.concatenate([pop[bits[s:s + 65536]].sum(axis=1, dtype=np.int32) for s in range(0, rows, 65536)])
    return bits, counts


def random_names(rng, count, length=31):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    blob = acgt[rng.integers(0, 4, size=count * length)]
    return blob, np.arange(count + 1, dtype=np.int64) * length


def stage_add(o):
    from pyseer_amd.enet import EnetPredictor
    from pyseer_amd.engine import Engine
    n = o.samples
    rng = np.random.default_rng(1)
    engine = Engine(n)
    start = rng.normal(size=n)
    for S in o.sizes:
        bits, _ = random_rows(rng, S, n)
        beta, flip, idx = rng.normal(size=S), (rng.random(S) < 0.3).astype(np.uint8), np.arange(S)
        pr = EnetPredictor(engine, start)
        pr.add(bits, idx[:1000], beta[:1000], flip[:1000])                      # warm-up: staging buffers, the kernel's code object
        ts = []
        for _ in range(o.repeats):
            t = time.perf_counter()
            pr.add(bits, idx, beta, flip)
            ts.append(time.perf_counter() - t)
        pr.finish()
        m = float(np.median(ts))
        emit(stage="add", samples=n, selected_rows=S, rows_per_s=S / m, staged_GB_per_s=S * (bits.shape[1] + 9) / m / 1e9, **stats(ts))
        del bits
    engine.close()


def stage_nameset(o):
    from pyseer_amd.enet import NameSet
    rng = np.random.default_rng(2)
    V, M, B = 1 << 20, 100000, 1 << 18
    blob, off = random_names(rng, V)
    picks = np.sort(rng.choice(V, size=M, replace=False))
    model = [bytes(blob[off[i]:off[i + 1]]).decode() for i in picks]
    ts, hits = [], 0
    for r in range(o.repeats + 1):
        ns = NameSet(model)                                                       # (a match retires its names: a fresh set per run)
        t = time.perf_counter()
        hits = 0
        for s in range(0, V, B):
            rows, _ = ns.match(blob[off[s]:off[min(s + B, V)]], off[s:min(s + B, V) + 1] - off[s])
            hits += rows.size
        dt = time.perf_counter() - t
        assert hits == M and ns.left == 0
        ns.close()
        if r:
            ts.append(dt)
    emit(stage="nameset", names=V, model_names=M, name_bytes=31, block=B, names_per_s=V / float(np.median(ts)), **stats(ts))


def _run_predict(args, repeats):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    ts = []
    for r in range(repeats + 1):
        t = time.perf_counter()
        res = subprocess.run([sys.executable, "-m", "pyseer_amd.enet_predict"] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        dt = time.perf_counter() - t
        assert res.returncode == 0, res.stderr.decode()[-2000:]
        if r:
            ts.append(dt)
    return ts, res.stdout


def _write_model(path, names, rng):
    from pyseer_amd.enet import write_model
    import collections
    model = collections.OrderedDict([("intercept", (1, 0.5))])
    for name in names:
        model[name] = (float(rng.uniform(0.01, 0.99)), float(rng.normal()))
    write_model(path, model, True)


def stage_cache(o):
    from pyseer_amd.input import PackedCacheWriter
    n, V, M, B = o.samples, o.cache_rows, o.cache_rows // 10, 1 << 18
    rng = np.random.default_rng(3)
    samples = ["s%d" % i for i in range(n)]
    with tempfile.TemporaryDirectory(dir=o.tmp) as tmp:
        cache, model, sfile = os.path.join(tmp, "bench.seerpack"), os.path.join(tmp, "model.txt"), os.path.join(tmp, "samples.txt")
        with open(sfile, "w") as fh:
            fh.write("\n".join(samples) + "\n")
        w = PackedCacheWriter(cache, samples)
        picked = []
        for s in range(0, V, B):
            rows = min(B, V - s)
            bits, counts = random_rows(rng, rows, n)
            blob, off = random_names(rng, rows)
            w.write_block(blob.tobytes(), off, counts, bits)
            picked += [bytes(blob[off[i]:off[i + 1]]).decode() for i in np.sort(rng.choice(rows, size=rows // 10, replace=False))]
        w.close()
        _write_model(model, picked, rng)
        ts, out = _run_predict([model, sfile, "--load-packed", cache], o.repeats)
        emit(stage="cache", samples=n, cache_rows=V, model_rows=len(picked), cache_bytes=os.path.getsize(cache), rows_per_s=V / float(np.median(ts)),
             output_lines=out.count(b"\n"), **stats(ts))


def stage_text(o):
    import gzip
    n, V = o.samples, o.text_lines
    rng = np.random.default_rng(4)
    tok = np.array([" s%d:1" % i for i in range(n)], dtype=object)
    acgt = np.array(list("ACGT"))
    af = np.where(rng.random(V) < 0.7, rng.uniform(0.01, 0.1, V), rng.uniform(0.1, 0.5, V))
    with tempfile.TemporaryDirectory(dir=o.tmp) as tmp:
        kmers, model, sfile = os.path.join(tmp, "kmers.gz"), os.path.join(tmp, "model.txt"), os.path.join(tmp, "samples.txt")
        with open(sfile, "w") as fh:
            fh.write("".join("s%d\n" % i for i in range(n)))
        names = []
        with gzip.open(kmers, "wt", compresslevel=1) as f:
            for s in range(0, V, 2000):
                K = rng.random((min(2000, V - s), n)) < af[s:s + 2000, None]
                nm = ["".join(acgt[x]) for x in rng.integers(0, 4, (K.shape[0], 31))]
                names += nm
                f.write("".join(nm[i] + " |" + "".join(tok[np.nonzero(K[i])[0]]) + "\n" for i in range(K.shape[0])))
        _write_model(model, [names[i] for i in np.sort(rng.choice(V, size=V // 10, replace=False))], rng)
        outs = {}
        for label, extra in (("native", []), ("python-reader", ["--python-reader"])):
            ts, outs[label] = _run_predict([model, sfile, "--kmers", kmers] + extra, o.repeats)
            emit(stage="text", reader=label, samples=n, lines=V, model_rows=V // 10, gz_bytes=os.path.getsize(kmers), lines_per_s=V / float(np.median(ts)), **stats(ts))
        assert outs["native"] == outs["python-reader"], "the two readers print different bytes"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--stage", choices=["add", "nameset", "cache", "text"], required=True)
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--sizes", type=int, nargs="*", default=[10000, 100000, 1000000])
    ap.add_argument("--cache-rows", type=int, default=1 << 20)
    ap.add_argument("--text-lines", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tmp", default=None, help="directory for the synthetic inputs")
    o = ap.parse_args()
    {"add": stage_add, "nameset": stage_nameset, "cache": stage_cache, "text": stage_text}[o.stage](o)


if __name__ == "__main__":
    main()
