"""tests/_dd_hash.py against itself: the scalar and the vectorised hash agree, the constructed rows collide and are distinct, the searched
rows have the home slots asked for, and the table's model counts what its definition says.  (That the restatement IS the device's hash is
held on the GPU: tests/test_dedup_collisions_gpu.py fails when the two differ.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dd_hash as H


def test_scalar_equals_vectorised():
    rng = np.random.default_rng(1)
    for n_words in (1, 2, 3, 5):
        rows = rng.integers(0, 1 << 64, size=(300, n_words), dtype=np.uint64)
        rows[0] = 0; rows[1] = np.uint64(H.M64)
        vec = H.hash_rows(rows)
        assert vec.dtype == np.uint64
        assert [int(x) for x in vec] == [H.hash_row(r) for r in rows]
    assert H.hash_rows(np.zeros((0, 2), dtype=np.uint64)).shape == (0,)


def test_mix_is_the_written_formula():
    """one step by hand, on numbers small enough to follow: h = 1, w = 2"""
    pre = 1 ^ ((2 + 0x9E3779B97F4A7C15 + (1 << 6) + (1 >> 2)) % 2 ** 64)
    mul = pre * 0xBF58476D1CE4E5B9 % 2 ** 64
    assert H.mix(1, 2) == mul ^ (mul >> 31)


def test_the_empty_marker_maps_to_zero():
    """a last word solved so that the mixing ends on the table's empty marker: the hash is 0, in both forms"""
    inv_mult = pow(H.MULT, -1, 1 << 64)
    x = H.DD_EMPTY
    x ^= x >> 31; x ^= x >> 62                                        # undo h ^= h >> 31
    pre = x * inv_mult % 2 ** 64
    h = H.mix(H.SEED, 12345)
    last = ((pre ^ h) - H.GOLD - ((h << 6) & H.M64) - (h >> 2)) & H.M64
    assert H.mix(h, last) == H.DD_EMPTY
    assert H.hash_row([12345, last]) == 0
    assert int(H.hash_rows(np.array([[12345, last]], dtype=np.uint64))[0]) == 0


@pytest.mark.parametrize("n_words", [2, 3])
def test_colliding_rows_are_distinct_with_one_hash(n_words):
    rows = H.colliding_rows(np.random.default_rng(10 + n_words), n_words, 6)
    assert rows.shape == (6, n_words) and rows.dtype == np.uint64
    assert len(np.unique(rows, axis=0)) == 6
    assert len(set(H.hash_row(r) for r in rows)) == 1
    assert len(np.unique(H.hash_rows(rows))) == 1
    # the solved last words look like any other: nothing near all-zero or all-one, so the rows sit well inside any AF window
    ones = [bin(int(w)).count("1") for w in rows[:, -1]]
    assert min(ones) >= 16 and max(ones) <= 48, ones


def test_home_slots_are_as_requested():
    rng = np.random.default_rng(5)
    rows, homes = H.rows_with_home_slot(rng, 2, 1024, [1023, 1022, 0, 1], [8, 4, 4, 4])
    assert rows.shape == (20, 2) and homes.tolist() == [1023] * 8 + [1022] * 4 + [0] * 4 + [1] * 4
    assert len(np.unique(rows, axis=0)) == 20
    assert ((H.hash_rows(rows) & np.uint64(1023)).astype(np.int64) == homes).all()
    assert len(np.unique(H.hash_rows(rows))) == 20                    # the low ten bits agree, the 64 do not
    rows3, homes3 = H.rows_with_home_slot(rng, 3, 256, [255], 2)
    assert rows3.shape == (2, 3) and [H.hash_row(r) & 255 for r in rows3] == [255, 255]


def test_probing_model_counts_the_keys_carried_past_the_end():
    # homes 6, 7, 7, 7, 0 in a table of 8: the second and third 7 go to slots 0 and 1, and the key at home in 0 moves to 2
    keys = [6, 7, 15, 23, 8]
    slot_of, wrapped = H.table_slots(np.array(keys + keys, dtype=np.uint64), 8)
    assert slot_of == {6: 6, 7: 7, 15: 0, 23: 1, 8: 2} and wrapped == 2
    assert H.table_slots(np.array(keys[::-1], dtype=np.uint64), 8)[1] == 2        # another order, other slots, as many carried over
    rows, _ = H.rows_with_home_slot(np.random.default_rng(6), 2, 1024, [1023], 8)
    assert H.table_slots(H.hash_rows(rows), 1024)[1] == 7


def test_model_of_the_table():
    rng = np.random.default_rng(8)
    fam = H.colliding_rows(rng, 2, 3)                                 # a, b, c: one hash
    other = rng.integers(0, 1 << 64, size=(2, 2), dtype=np.uint64)    # p, q
    a, b, c = fam; p, q = other
    rows = np.array([p, b, a, b, q, a, c, p, b], dtype=np.uint64)
    rep, n = H.expected_representatives(rows)
    # row 1 (b) owns the family's hash: its copies fold into it; a and c differ from the owner, so every copy of them stands alone
    assert rep.tolist() == [0, 1, 2, 1, 4, 5, 6, 0, 1]
    assert n == 6 and len(np.unique(rows, axis=0)) == 5
    rep, n = H.expected_representatives(rows[::-1])                   # reversed, a b comes first again
    assert n == len(rows) - 2 - 1                                     # three b's fold into one, two p's into one


def test_words_and_dense_round_trip():
    rng = np.random.default_rng(2)
    for N in (64, 128, 130, 192):
        K = (rng.random((17, N)) < 0.5).astype(np.uint8)
        w = H.words_of(K)
        assert w.shape == (17, (N + 63) // 64) and np.array_equal(H.dense_of(w, N), K)
    assert int(H.words_of(np.array([[1, 0, 1] + [0] * 61 + [1]]))[0, 0]) == 5 and int(H.words_of(np.array([[1, 0, 1] + [0] * 61 + [1]]))[0, 1]) == 1
