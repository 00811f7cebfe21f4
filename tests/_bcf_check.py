"""Shared by the BCF tests: the records of a file as (names, skip reasons, present rows, missing rows, present counts, missing counts) from a
Python reader (VcfFile on text, BcfFile on BCF) and from the native reader, and their comparison."""
import collections
import contextlib
import io

import numpy as np


def python_records(f, samples):
    from pyseer_amd.packing import pack_variants
    names, skip, pres, miss = [], [], [], []
    keep = set(samples)
    with contextlib.redirect_stderr(io.StringIO()):
        for rec in f:
            d = {}
            f.apply(rec, d)
            names.append(rec.name); skip.append(rec.skip)
            pres.append([1 if (s in keep and d.get(s) == 1) else 0 for s in samples])
            miss.append([1 if (s in d and d[s] != 1) else 0 for s in samples])
    pres, miss = np.array(pres, dtype=np.uint8).reshape(len(names), len(samples)), np.array(miss, dtype=np.uint8).reshape(len(names), len(samples))
    return names, np.array(skip), pack_variants(pres), pack_variants(miss), pres.sum(axis=1), miss.sum(axis=1)


def native_records(path, samples, engine, block_size):
    """The same six, and the reader's info(), through sh_vcf_* (engine None: the library's host restatement of the kernel)."""
    from pyseer_amd.input import NativeVcfReader
    r = NativeVcfReader(path, samples, engine, block_size)
    names, parts = [], collections.defaultdict(list)
    try:
        for rb in r.raw_blocks():
            assert 1 <= len(rb["skip"]) <= block_size
            names += [rb["blob"][rb["off"][i]:rb["off"][i + 1]].decode() for i in range(len(rb["skip"]))]
            for key in ("skip", "present", "missing", "n_present", "n_missing", "pos", "ref_len"):
                parts[key].append(rb[key].copy())
        info = r.info()
    finally:
        r.close()
    if not names:
        return [], info
    return (names,) + tuple(np.concatenate(parts[k]) for k in ("skip", "present", "missing", "n_present", "n_missing", "pos", "ref_len")) + (info,)


def assert_same(got, want, what):
    assert list(got[0]) == list(want[0]), "%s: names" % what
    for j, thing in ((1, "skip reasons"), (2, "present rows"), (3, "missing rows"), (4, "present counts"), (5, "missing counts")):
        if not np.array_equal(got[j], want[j]):
            bad = np.nonzero(np.asarray(got[j] != want[j]).reshape(len(want[0]), -1).any(axis=1))[0]
            raise AssertionError("%s: %s differ, first at record %d (%s)" % (what, thing, int(bad[0]), want[0][int(bad[0])]))
