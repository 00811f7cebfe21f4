"""The host side of --wg enet's native VCF route without a device: input.iter_call_blocks_vcf_native over the reader's host restatement
of its kernel (engine=None), enet.load_all_vars_calls, KeptCalls.take and selected_from_rows with missing calls.

The device matrix is replaced by a numpy stand-in that applies the stated rule (include/seerhip.h, sh_enet_ingest_calls), so what is
checked here is what the host makes of the blocks: the messages and their order, the stream indices, the names, the counts, the missing
rows it keeps, and read_variant's tuple recovered from a stored row.  The yardstick is read_variant line by line (enet.load_all_vars).
tests/test_enet_calls_gpu.py and tests/test_enet_vcf_native_gpu.py hold the device code and the command line."""
import io
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vcf_text  # noqa: E402


class NumpyMatrix(object):
    """EnetMatrix's append / ingest_calls / get_rows in numpy"""

    def __init__(self, engine, capacity):
        from pyseer_amd.packing import row_bytes_for
        self.n = engine.n
        self.row_bytes = row_bytes_for(self.n)
        self.R = np.zeros((0, self.row_bytes), dtype=np.uint8)
        tail = np.zeros(self.row_bytes * 8, dtype=np.uint8)
        tail[:self.n] = 1
        self.valid = np.packbits(tail, bitorder="little")

    rows = property(lambda self: self.R.shape[0])

    def close(self):
        pass

    def append(self, present, missing=None, flip=None):
        rows = present.copy()
        f = np.asarray(flip).astype(bool)
        rows[f] = ~rows[f] & ~missing[f]
        self.R = np.concatenate([self.R, rows & self.valid])

    def ingest_calls(self, present, missing, skip, lo, hi, mm):
        P, Mi = present & self.valid, missing & self.valid
        c = np.unpackbits(P, axis=1).sum(axis=1)
        m = np.unpackbits(Mi & ~P, axis=1).sum(axis=1)
        t = c + m
        idx = np.nonzero((np.asarray(skip) == 0) & (t >= lo) & (t <= hi) & (m <= mm))[0]
        self.append(P[idx], Mi[idx], 2 * t[idx] > self.n)
        return idx.astype(np.int32), c[idx].astype(np.int32), m[idx].astype(np.int32)

    def get_rows(self, idx):
        return self.R[np.asarray(idx, dtype=np.int64)]


class _Engine(object):
    def __init__(self, n):
        self.n = n


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """600 generated records over 200 phenotyped samples among 230 columns, 3 % missing calls; read_variant's tuple of every record"""
    from pyseer_amd import input as inp
    text, pheno, _ = _vcf_text.generated_vcf(n_pheno=200, n_cols=230, n_records=600, seed=7, missing=0.03)
    path = str(tmp_path_factory.mktemp("enet_calls") / "generated.vcf.gz")
    _vcf_text.write_bgzf(path, text)
    p = pd.Series(np.arange(200) % 2, index=pheno)
    infile, order = inp.open_variant_file("vcf", path)
    old, sys.stderr = sys.stderr, io.StringIO()
    try:
        tuples = [inp.read_variant(infile, p, "vcf", False, None, False, set(p.index), order) for _ in range(600)]
        said = sys.stderr.getvalue()
    finally:
        sys.stderr = old
    return path, p, tuples, said


@pytest.mark.parametrize("block", [7, 64, 4096])
def test_loader_over_call_blocks_is_the_line_by_line_loader(block, generated, monkeypatch):
    from pyseer_amd import enet
    from pyseer_amd import input as inp
    path, p, tuples, said = generated
    monkeypatch.setattr(enet, "EnetMatrix", NumpyMatrix)
    n = len(p)
    infile, order = inp.open_variant_file("vcf", path)
    monkeypatch.setattr(sys, "stderr", io.StringIO())
    M1, vi1, loaded1 = enet.load_all_vars(_Engine(n), "vcf", p, False, None, infile, set(p.index), order, 0.01, 0.99, 0.05, False)
    said1 = sys.stderr.getvalue()
    err = io.StringIO()
    M2, vi2, loaded2, kept = enet.load_all_vars_calls(_Engine(n), p, inp.iter_call_blocks_vcf_native(p, path, None, block), 0.01, 0.99, 0.05, err)
    assert loaded1 == loaded2 == 600 and list(vi1) == list(vi2) and len(vi2) == 458
    assert (M1.R == M2.R).all()
    assert err.getvalue() == said1 == said and said.count("Multiple alleles at ") > 0 and said.count("No observations of ") > 0
    flipped = 2 * kept.counts > n
    assert int(kept.has_missing.sum()) == 442 == kept.missing_rows.shape[0] and int(flipped.sum()) == 98 and int((flipped & kept.has_missing).sum()) == 95
    names = [bytes(kept.blob[kept.off[i]:kept.off[i + 1]]).decode() for i in range(458)]
    assert names == [tuples[i][2] for i in vi2]
    assert (kept.counts == [len(tuples[i][3]) for i in vi2]).all()
    # a cut (the correlation filter's, the selection's) takes names, counts, missing rows and messages together; the selected rows give
    # read_variant's tuples back: k (int without a missing call, float with NaN where there is one), af, the two sample lists
    sel = np.concatenate([np.arange(3, 458, 7), np.nonzero(~kept.has_missing)[0]])
    sel = np.unique(sel)
    cut = kept.take(sel)
    monkeypatch.setattr(enet, "_enet_row", lambda name, k, af, ks, nks, *rest: (name, k, af, ks, nks))
    got = list(enet.selected_from_rows(np.ones(sel.size), M2.get_rows(sel), (cut.blob, cut.off), cut.counts, p, None, None, False, False, None, io.StringIO(),
                                       missing_rows=cut.missing_list(), messages=cut.messages))
    kinds = set()
    for j, (name, k, af, ks, nks) in enumerate(got):
        _, k0, name0, ks0, nks0, af0, miss0 = tuples[vi2[sel[j]]]
        assert name == name0 and af == af0 and ks == ks0 and nks == nks0
        assert k.dtype == k0.dtype and np.array_equal(k, k0, equal_nan=True)
        kinds.add((bool(flipped[sel[j]]), miss0 > 0))
    assert len(kinds) == 4                                            # stored as it is or by its absences, with and without a missing call


def test_messages_of_a_selected_variant_are_written_again():
    from pyseer_amd import enet
    n, rb = 10, 8
    p = pd.Series(np.zeros(n), index=["s%d" % i for i in range(n)])
    rows = np.zeros((2, rb), dtype=np.uint8)
    rows[0, 0] = 0b00000111
    miss = np.zeros(rb, dtype=np.uint8)
    miss[1] = 0b00000010                                              # sample 9
    err = io.StringIO()
    orig = enet._enet_row
    enet._enet_row = lambda name, k, af, ks, nks, *rest: (name, k, af, ks, nks)
    try:
        got = list(enet.selected_from_rows(np.ones(2), rows, (np.frombuffer(b"AB", dtype=np.uint8), np.array([0, 1, 2])), np.array([4, 0]), p, None, None, False,
                                           False, None, err, missing_rows=[miss, None], messages=["Could not parse region None\n", ""]))
    finally:
        enet._enet_row = orig
    assert err.getvalue() == "Could not parse region None\nNo observations of B in selected samples\n"
    name, k, af, ks, nks = got[0]
    assert name == "A" and af == 0.4 and ks == ["s0", "s1", "s2", "s9"] and len(nks) == 6
    assert np.array_equal(k, [1, 1, 1, 0, 0, 0, 0, 0, 0, np.nan], equal_nan=True)
    assert got[1][1].dtype == np.int64 and not got[1][1].any()


def test_the_packed_block_stream_is_unchanged_by_the_shared_call_blocks(generated):
    """iter_packed_blocks_vcf_native is built on the same CallBlocks: it still gives what iter_packed_blocks gives from read_variant."""
    from pyseer_amd import input as inp
    path, p, tuples, said = generated
    for block in (7, 4096):
        old, sys.stderr = sys.stderr, io.StringIO()
        try:
            infile, order = inp.open_variant_file("vcf", path)
            a = list(inp.iter_packed_blocks(p, "vcf", infile, set(p.index), order, 0.01, 0.99, 0.05, False, block))
            said_a, sys.stderr = sys.stderr.getvalue(), io.StringIO()
            b = list(inp.iter_packed_blocks_vcf_native(p, path, None, 0.01, 0.99, 0.05, block))
            said_b = sys.stderr.getvalue()
        finally:
            sys.stderr = old
        assert said_a == said_b and len(a) == len(b)
        for x, y in zip(a, b):
            assert list(x.names) == list(y.names) and x.status == y.status and x.patterns == y.patterns and x.row_of == y.row_of
            assert np.array_equal(np.asarray(x.afs, dtype=float), np.asarray(y.afs, dtype=float), equal_nan=True)
            assert (x.bits == y.bits).all()
