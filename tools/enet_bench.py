#!/usr/bin/env python
"""Times the whole-genome elastic net on synthetic k-mers (the benchmark's AF mix): upload, the correlation pass (k_enet_moments: it reads
every row once, so its rate against the HBM roof is the yardstick of the streaming kernels), and the cross-validated fit (k_enet_cd
coordinate steps per second, KKT rounds).  One JSON line per measurement; warm-up run first, then --repeats timed runs (median, min, max).

    python tools/enet_bench.py --variants 100000 --samples 5000 --n-lambda 5

--ingest times the load path of k-mer input instead: sh_enet_ingest alone on 2^18-row blocks of host memory with about half the rows
kept, then enet.load_all_vars_blocks (the command line's load stage up to the correlations) from a packed cache written here, next to the
bare walk over the cache's blocks.  --load-kmers FILE times the same stage from a gzipped k-mer text (--python-reader: through
enet.load_all_vars, the line-by-line path) and reports the process's peak resident set.

    python tools/enet_bench.py --ingest --variants 1048576 --samples 5000
    python tools/enet_bench.py --write-kmers kmers.gz --variants 100000 --samples 5000          # synthetic text + kmers.gz.pheno
    python tools/enet_bench.py --load-kmers kmers.gz --pheno kmers.gz.pheno [--python-reader]

--load-vcf FILE times the same stage from a VCF: the native reader alone (sh_vcf_stats), enet.load_all_vars_calls (the command line's route
for --vcf), and sh_enet_ingest_calls alone on blocks of the file held in host memory; --python-reader: enet.load_all_vars line by line, on
the whole FILE, so give it a prefix.  --write-vcf DIR generates the input from a seed (tools/bench_vcf_reader.py's generator: N = 5000
phenotyped samples among 5200 columns, 3 % missing calls): DIR/gen.vcf.gz of --variants records (BGZF), DIR/first.vcf (its first 2000
records, plain text) and DIR/gen.pheno.

    python tools/enet_bench.py --write-vcf DIR --variants 200000
    python tools/enet_bench.py --load-vcf DIR/gen.vcf.gz --pheno DIR/gen.pheno
    python tools/enet_bench.py --load-vcf DIR/first.vcf --pheno DIR/gen.pheno --python-reader"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synth(P, N, seed):
    rng = np.random.default_rng(seed)
    af = np.where(rng.random(P) < 0.7, rng.uniform(0.01, 0.1, P), rng.uniform(0.1, 0.5, P))
    rows = np.zeros((P, ((N + 63) // 64) * 8), np.uint8)
    for s in range(0, P, 20000):                                     # in slabs: the unpacked matrix of 1e7 rows does not fit a host
        K = rng.random((min(20000, P - s), N)) < af[s:s + 20000, None]
        pk = np.packbits(K, axis=1, bitorder="little")
        rows[s:s + pk.shape[0], :pk.shape[1]] = pk
    return rows


def stats(ts):
    return dict(median_s=float(np.median(ts)), min_s=float(np.min(ts)), max_s=float(np.max(ts)), n=len(ts))


def peak_rss_mb():
    import resource
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0


def ingest_stage(o):
    import tempfile
    import pandas as pd
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix, load_all_vars_blocks
    from pyseer_amd.input import PackedCacheWriter, iter_packed_blocks_cached
    P, N, B = o.variants, o.samples, 1 << 18
    rows = synth(P, N, 1)
    counts = np.concatenate([np.unpackbits(rows[s:s + 20000], axis=1, bitorder="little").sum(axis=1) for s in range(0, P, 20000)]).astype(np.int32)
    lo, hi = int(np.median(counts)), N                                # about half the rows are kept
    kept = int(((counts >= lo) & (counts <= hi)).sum())
    e = Engine(N)
    ts = []
    for r in range(o.repeats + 1):
        M = EnetMatrix(e, kept)                                       # (no growth inside the timed part: that is the next line's)
        t = time.perf_counter()
        for s in range(0, P, B):
            M.ingest(rows[s:s + B], lo, hi)
        dt = time.perf_counter() - t
        assert M.rows == kept
        M.close()
        if r:
            ts.append(dt)
    med = float(np.median(ts))
    print(json.dumps(dict(what="sh_enet_ingest, 2^18-row blocks of host memory, capacity reserved", variants=P, samples=N, kept=kept, bytes=int(rows.nbytes),
                          rows_per_s=P / med, gb_per_s=rows.nbytes / med / 1e9, **stats(ts))), flush=True)
    ts = []
    for r in range(o.repeats + 1):
        M = EnetMatrix(e, 1)
        t = time.perf_counter()
        for s in range(0, P, B):
            M.ingest(rows[s:s + B], lo, hi)
        dt = time.perf_counter() - t
        M.close()
        if r:
            ts.append(dt)
    med = float(np.median(ts))
    print(json.dumps(dict(what="sh_enet_ingest, the same from an initial capacity of 1 (the matrix grows)", variants=P, samples=N, kept=kept,
                          rows_per_s=P / med, gb_per_s=rows.nbytes / med / 1e9, **stats(ts))), flush=True)
    # the same rows as a packed cache (page cache warm after the write): the bare walk over its blocks, touching one byte per page, and the load
    names = ("K%09d" % 0).encode()
    p = pd.Series(np.zeros(N), index=["s%d" % i for i in range(N)])
    with tempfile.TemporaryDirectory(dir=o.tmp) as d:
        path = os.path.join(d, "bench.seerpack")
        w = PackedCacheWriter(path, list(p.index))
        for s in range(0, P, B):
            nv = min(B, P - s)
            w.write_block(names * nv, np.arange(nv + 1, dtype=np.int64) * len(names), counts[s:s + nv], rows[s:s + nv])
        w.close()
        ts = []
        for r in range(o.repeats + 1):
            t = time.perf_counter(); tot = 0
            for blk in iter_packed_blocks_cached(p, path, 0.0, 1.0, B, raw=True, device=None):
                tot += int(blk.bits.reshape(-1)[::4096].sum())
            dt = time.perf_counter() - t
            if r:
                ts.append(dt)
        med = float(np.median(ts))
        print(json.dumps(dict(what="packed cache: walk over the blocks, one byte per page read", variants=P, samples=N, rows_per_s=P / med,
                              gb_per_s=rows.nbytes / med / 1e9, **stats(ts))), flush=True)
        min_af = (lo - 0.5) / N
        ts = []
        for r in range(o.repeats + 1):
            t = time.perf_counter()
            M, vi, loaded, _, _, _ = load_all_vars_blocks(e, p, iter_packed_blocks_cached(p, path, 0.0, 1.0, B, raw=True, device=None), min_af, 1.1, 0.05)
            dt = time.perf_counter() - t
            assert loaded == P and M.rows == kept
            M.close()
            if r:
                ts.append(dt)
        med = float(np.median(ts))
        print(json.dumps(dict(what="load_all_vars_blocks from the packed cache (reader thread + ingest + names and counts)", variants=P, samples=N,
                              kept=kept, rows_per_s=P / med, gb_per_s=rows.nbytes / med / 1e9, peak_rss_mb=peak_rss_mb(), **stats(ts))), flush=True)
    e.close()


def write_kmers(o):
    """--write-kmers FILE: --variants lines of gzipped k-mer text over --samples samples s0, s1, ... (synth()'s AF mix), and FILE.pheno."""
    import gzip
    N, P = o.samples, o.variants
    rng = np.random.default_rng(7)
    tok = np.array([" s%d:1" % i for i in range(N)], dtype=object)
    af = np.where(rng.random(P) < 0.7, rng.uniform(0.01, 0.1, P), rng.uniform(0.1, 0.5, P))
    acgt = np.array(list("ACGT"))
    with gzip.open(o.write_kmers, "wt", compresslevel=1) as f:
        for s in range(0, P, 2000):
            K = rng.random((min(2000, P - s), N)) < af[s:s + 2000, None]
            names = rng.integers(0, 4, (K.shape[0], 31))
            f.write("".join("".join(acgt[names[i]]) + " |" + "".join(tok[np.nonzero(K[i])[0]]) + "\n" for i in range(K.shape[0])))
    with open(o.write_kmers + ".pheno", "w") as f:
        f.write("samples\tbinary\n" + "".join("s%d\t%d\n" % (i, b) for i, b in enumerate(rng.integers(0, 2, N))))


def load_kmers_stage(o):
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import load_all_vars, load_all_vars_blocks
    from pyseer_amd.input import iter_packed_blocks_native, load_phenotypes, open_variant_file
    p = load_phenotypes(o.pheno, None)
    e = Engine(len(p))
    t = time.perf_counter()
    if o.python_reader:
        infile, order = open_variant_file("kmers", o.load_kmers)
        M, vi, loaded = load_all_vars(e, "kmers", p, False, None, infile, set(p.index), order, 0.01, 0.99, 0.05, False)
    else:
        M, vi, loaded = load_all_vars_blocks(e, p, iter_packed_blocks_native(p, o.load_kmers, 0.0, 1.0, 1 << 18, raw=True), 0.01, 0.99, 0.05)[:3]
    dt = time.perf_counter() - t
    t = time.perf_counter(); M.correlations(p.values.astype(float)); dc = time.perf_counter() - t
    print(json.dumps(dict(what="load stage from gzipped k-mer text, %s" % ("load_all_vars (--python-reader)" if o.python_reader else "native reader + load_all_vars_blocks"),
                          lines=int(loaded), kept=int(M.rows), samples=len(p), seconds=dt, lines_per_s=loaded / dt, correlations_s=dc,
                          peak_rss_mb=peak_rss_mb())), flush=True)
    M.close()
    e.close()


def write_vcf(o):
    """--write-vcf DIR: the generated call set of tools/bench_vcf_reader.py with --variants records, and DIR/gen.pheno for its 5000 samples."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from bench_vcf_reader import make_file
    path, meta = make_file(o.write_vcf, None, records=o.variants)
    rng = np.random.default_rng(7)
    with open(os.path.join(o.write_vcf, "gen.pheno"), "w") as f:
        f.write("samples\tbinary\n" + "".join("%s\t%d\n" % (s, b) for s, b in zip(meta["samples"], rng.integers(0, 2, len(meta["samples"])))))
    print(json.dumps(dict(what="generated VCF", path=path, records=meta["records"], text_GB=meta["text_bytes"] / 1e9, file_MB=meta["file_bytes"] / 1e6)), flush=True)


def load_vcf_stage(o):
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix, call_bounds, load_all_vars, load_all_vars_calls
    from pyseer_amd.input import NativeVcfReader, iter_call_blocks_vcf_native, load_phenotypes, open_variant_file
    p = load_phenotypes(o.pheno, None)
    n, B = len(p), o.vcf_block
    e = Engine(n)
    devnull = open(os.devnull, "w")
    if o.python_reader:
        import contextlib
        t = time.perf_counter()
        infile, order = open_variant_file("vcf", o.load_vcf)
        with contextlib.redirect_stderr(devnull):
            M, vi, loaded = load_all_vars(e, "vcf", p, False, None, infile, set(p.index), order, 0.01, 0.99, 0.05, False)
        dt = time.perf_counter() - t
        print(json.dumps(dict(what="load stage from a VCF, load_all_vars (--python-reader)", records=int(loaded), kept=int(M.rows), samples=n, seconds=dt,
                              records_per_s=loaded / dt, peak_rss_mb=peak_rss_mb())), flush=True)
        M.close()
        e.close()
        return
    # the reader alone, twice (the first pass also pays the page cache and the pinned slabs); the blocks of the first --ingest-records stay
    held, dt_reader = [], 0.0
    for rep in range(2):
        r = NativeVcfReader(o.load_vcf, [str(x) for x in p.index], e, B)
        t = time.perf_counter(); nrec = 0; held = []
        for rb in r.raw_blocks():
            if nrec < o.ingest_records:
                held.append((rb["present"], rb["missing"], rb["skip"]))
            nrec += rb["skip"].shape[0]
        dt_reader = time.perf_counter() - t
        st = r.stats()
        r.close()
        print(json.dumps(dict(what="native VCF reader alone, pass %d" % (rep + 1), records=nrec, samples=n, block=B, seconds=dt_reader, records_per_s=nrec / dt_reader,
                              sample_bytes=st["sample_bytes"], launches=st["launches"])), flush=True)
    ts = []
    for rep in range(o.repeats + 1):
        t = time.perf_counter()
        M, vi, loaded, kept = load_all_vars_calls(e, p, iter_call_blocks_vcf_native(p, o.load_vcf, e, B), 0.01, 0.99, 0.05, devnull)
        dt = time.perf_counter() - t
        rows, with_missing = int(M.rows), int(kept.has_missing.sum())
        if rep:
            ts.append(dt)
        if rep < o.repeats:
            M.close()
    med = float(np.median(ts))
    t = time.perf_counter(); M.correlations(p.values.astype(float)); dc = time.perf_counter() - t
    M.close()
    print(json.dumps(dict(what="load stage from a VCF, native reader + load_all_vars_calls", records=int(loaded), kept=rows, kept_with_missing=with_missing,
                          samples=n, block=B, records_per_s=loaded / med, reader_alone_share=dt_reader / med, correlations_s=dc,
                          missing_rows_held_mb=with_missing * M.row_bytes / 1e6, peak_rss_mb=peak_rss_mb(), **stats(ts))), flush=True)
    # sh_enet_ingest_calls alone: the held blocks from host memory, the matrix's capacity reserved
    lo, hi, mm = call_bounds(n, 0.01, 0.99, 0.05)
    nheld = sum(b[2].shape[0] for b in held)
    ts = []
    for rep in range(o.repeats + 1):
        M = EnetMatrix(e, nheld)
        t = time.perf_counter()
        for pres, miss, skip in held:
            M.ingest_calls(pres, miss, skip, lo, hi, mm)
        dt = time.perf_counter() - t
        rows = int(M.rows)
        M.close()
        if rep:
            ts.append(dt)
    med = float(np.median(ts))
    nbytes = 2 * nheld * held[0][0].shape[1]
    print(json.dumps(dict(what="sh_enet_ingest_calls alone, %d-record blocks of host memory, capacity reserved (host clock around the synchronous calls)" % B,
                          records=nheld, kept=rows, samples=n, bytes=nbytes, records_per_s=nheld / med, gb_per_s=nbytes / med / 1e9, **stats(ts))), flush=True)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ingest", action="store_true", help="the load path: sh_enet_ingest alone and from a packed cache")
    ap.add_argument("--load-kmers", default=None, help="time the load stage from this gzipped k-mer file (needs --pheno)")
    ap.add_argument("--pheno", default=None)
    ap.add_argument("--write-kmers", default=None, help="write --variants lines of synthetic gzipped k-mer text (and FILE.pheno) and stop: no device needed")
    ap.add_argument("--load-vcf", default=None, help="time the load stage from this VCF (needs --pheno)")
    ap.add_argument("--write-vcf", default=None, help="write DIR/gen.vcf.gz of --variants generated records, DIR/first.vcf and DIR/gen.pheno and stop: no device needed")
    ap.add_argument("--vcf-block", type=int, default=1 << 14, help="records per block of --load-vcf (the command line's: max(--block_size, 2^14))")
    ap.add_argument("--ingest-records", type=int, default=1 << 16, help="records of --load-vcf held in memory for the timing of sh_enet_ingest_calls alone")
    ap.add_argument("--python-reader", action="store_true")
    ap.add_argument("--tmp", default=None, help="directory for the packed cache of --ingest")
    ap.add_argument("--variants", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--n-folds", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.0069)
    ap.add_argument("--n-lambda", type=int, default=100)
    ap.add_argument("--thresh", type=float, default=1e-7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-fit", action="store_true", help="the streaming kernels only")
    ap.add_argument("--continuous", action="store_true")
    o = ap.parse_args()
    if o.write_kmers:
        return write_kmers(o)
    if o.ingest:
        return ingest_stage(o)
    if o.load_kmers:
        return load_kmers_stage(o)
    if o.write_vcf:
        return write_vcf(o)
    if o.load_vcf:
        return load_vcf_stage(o)
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import EnetMatrix, assign_folds
    P, N = o.variants, o.samples
    rows = synth(P, N, 1)
    rng = np.random.default_rng(2)
    K10 = np.unpackbits(rows[:10], axis=1, bitorder="little")[:, :N].astype(float)
    lin = K10.T @ rng.normal(0, 1, 10)
    y = lin + rng.normal(0, 1, N) if o.continuous else (rng.random(N) < 1 / (1 + np.exp(-(lin - np.median(lin))))).astype(float)
    e = Engine(N)
    ts = []
    for r in range(o.repeats + 1):
        M = EnetMatrix(e, P)
        t = time.perf_counter(); M.append(rows); dt = time.perf_counter() - t
        if r:
            ts.append(dt)
        if r < o.repeats:
            M.close()
    print(json.dumps(dict(what="upload", variants=P, samples=N, bytes=int(rows.nbytes), gb_per_s=rows.nbytes / np.median(ts) / 1e9, **stats(ts))), flush=True)
    M.correlations(y)
    ts = []
    for r in range(o.repeats):
        t = time.perf_counter(); M.correlations(y); ts.append(time.perf_counter() - t)
    print(json.dumps(dict(what="correlations (k_enet_moments + copy of the result)", variants=P, samples=N, row_bytes_read=int(rows.nbytes),
                          gb_per_s=rows.nbytes / np.median(ts) / 1e9, hbm_roof_gb_per_s=8000, **stats(ts))), flush=True)
    V = rng.normal(size=(o.n_folds + 1, N))
    M.carrier_sums(V)
    ts = []
    for r in range(o.repeats):
        t = time.perf_counter(); M.carrier_sums(V); ts.append(time.perf_counter() - t)
    print(json.dumps(dict(what="carrier sums of %d vectors (k_enet_grad + upload of the vectors + copy of the %d x P result)" % (V.shape[0], V.shape[0]),
                          variants=P, samples=N, row_bytes_read=int(rows.nbytes), result_bytes=int(8 * V.shape[0] * P),
                          gb_per_s_of_rows=rows.nbytes / np.median(ts) / 1e9, hbm_roof_gb_per_s=8000, **stats(ts))), flush=True)
    if not o.no_fit:
        fold = assign_folds(N, o.n_folds, 1)
        t = time.perf_counter()
        fit = M.fit(y, o.continuous, o.alpha, fold_id=fold, n_folds=o.n_folds, thresh=o.thresh, n_lambda=o.n_lambda)
        dt = time.perf_counter() - t
        print(json.dumps(dict(what="fit", variants=P, samples=N, n_folds=o.n_folds, alpha=o.alpha, thresh=o.thresh, n_lambda_asked=o.n_lambda,
                              n_lambda_fitted=fit.n_lambda, seconds=dt, kkt_rounds=fit.kkt_rounds, cd_sweeps=int(fit.cd_sweeps),
                              cd_steps=int(fit.cd_steps), cd_steps_per_s_of_the_whole_fit=fit.cd_steps / dt, state_in_lds=fit.state_in_lds,
                              nzero_last=int(fit.nzero[-1]), i_min=fit.i_min)), flush=True)
    M.close()
    e.close()


if __name__ == "__main__":
    main()
