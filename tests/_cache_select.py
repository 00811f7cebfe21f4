"""Shared by tests/test_cache_select_cpu.py and tests/test_cache_select_gpu.py: the numpy yardstick of the row selection (unpackbits -> fancy
index -> packbits), the shapes and maps both suites walk, and the fixture's full sample list."""
import gzip
import os

import numpy as np

from pyseer_amd.packing import row_bytes_for

CLI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli")

N_SRC = (1, 8, 63, 64, 65, 1837, 5200)
V_ROWS = (0, 1, 257)
MAP_KINDS = ("identity", "reversed", "subset", "permuted")


def n_dsts(n_src):
    return sorted({d for d in (1, 7, 64, 65, n_src) if d <= n_src})


def make_map(kind, n_src, n_dst, rng):
    """identity / reversed: the first / last n_dst source bits, in / against their order; subset: a random subset in the source's order;
    permuted: a random subset in random order."""
    if kind == "identity":
        m = np.arange(n_dst)
    elif kind == "reversed":
        m = np.arange(n_src - 1, n_src - 1 - n_dst, -1)
    elif kind == "subset":
        m = np.sort(rng.choice(n_src, n_dst, replace=False))
    else:
        m = rng.permutation(n_src)[:n_dst]
    return m.astype(np.int32)


def source_rows(V, n_src, rng, density=0.3):
    """(V, row_bytes_for(n_src)) packed rows whose padding bits are all ONES, and the dense 0/1 matrix they hold."""
    dense = (rng.random((V, n_src)) < density).astype(np.uint8)
    rb = row_bytes_for(n_src)
    full = np.ones((V, rb * 8), dtype=np.uint8)
    full[:, :n_src] = dense
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")), dense


def numpy_select(bits, n_src, sample_map):
    """-> (rows, counts) by unpackbits -> fancy index -> packbits; padding bits of the result are zero"""
    dense = np.unpackbits(np.ascontiguousarray(bits), axis=1, bitorder="little")[:, :n_src][:, sample_map]
    out = np.zeros((bits.shape[0], row_bytes_for(len(sample_map))), dtype=np.uint8)
    packed = np.packbits(dense, axis=1, bitorder="little")
    out[:, :packed.shape[1]] = packed
    return out, dense.sum(axis=1).astype(np.int32)


def check_selected(got_bits, got_counts, bits, n_src, sample_map):
    want_bits, want_counts = numpy_select(bits, n_src, sample_map)
    n_dst = len(sample_map)
    assert got_bits.shape == want_bits.shape and got_bits.dtype == np.uint8
    assert np.array_equal(got_bits, want_bits)                                    # (whole rows: the padding bits are zero in both)
    pad = np.unpackbits(np.ascontiguousarray(got_bits), axis=1, bitorder="little")[:, n_dst:]
    assert not pad.any()
    assert got_counts.dtype == np.int32 and np.array_equal(got_counts, want_counts)


def all_samples():
    """every sample kmers.gz names, sorted (1837)"""
    names = set()
    with gzip.open(os.path.join(CLI, "kmers.gz"), "rt") as fh:
        for line in fh:
            names.update(tok.rsplit(":", 1)[0] for tok in line.split("|", 1)[1].split())
    return sorted(names)


def phenotype(name, column=-1):
    import pandas as pd
    p = pd.read_csv(os.path.join(CLI, name), index_col=0, sep="\t")
    p.index = p.index.astype(str)
    return p[p.columns[column]]
