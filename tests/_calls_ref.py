"""What tests/test_calls_job_cpu.py and tests/test_calls_job_gpu.py share: the float64 md5 of a row with missing calls restated from the message
words k_job_md5_calls builds (csrc/job_kernels.hip), and the generator of the call blocks Job.submit_calls is held to the host route on."""
import base64
import hashlib
import struct

import numpy as np

V = 257                                                    # crosses a workgroup of k_job_count's 256 threads, and of k_job_md5_calls
SIZES = (15, 63, 64, 65, 127)                              # N % 8 == 7 (the marker in a block of its own) and both sides of a 64-bit word


def f64_pattern(present, missing):
    """base64(md5) + newline of the float64 vector hash_pattern sees for a variant with missing calls, built word by word as the kernel builds
    it: per sample a zero low word, then 0x7FF80000 (numpy's nan) where the call is missing, 0x3FF00000 (1.0) where it is present, else zero."""
    words = []
    for p, m in zip(present, missing):
        words += [0, 0x7FF80000 if m else (0x3FF00000 if p else 0)]
    return base64.b64encode(hashlib.md5(struct.pack("<%dI" % len(words), *words)).digest()) + b"\n"


def make_case(N, continuous, seed):
    """One call block of V records over N samples with every edge the marking kernel has (the row numbers are fixed, the rest is random):
    skipped records first, in the middle and last; af exactly at both ends of the window and one carrier outside, with and without the help of
    a missing call; the missing rate exactly at max_missing and one call above; every call missing; no carrier among the called samples
    (an empty margin: filter-pvalue NaN); rows with no, one and several missing calls."""
    rng = np.random.default_rng(seed)
    a, b, mm = 2, N - 3, 2
    case = {"N": N, "min_af": float(a) / N, "max_af": float(b) / N, "max_missing": float(mm) / N}
    if continuous:
        y = rng.standard_normal(N)
    else:
        y = (np.arange(N) % 2).astype(float)
        rng.shuffle(y)
    P = np.zeros((V, N), dtype=np.uint8); M = np.zeros((V, N), dtype=np.uint8)
    skip = np.zeros(V, dtype=np.int32)
    skip[[0, V // 2, V - 1]] = 1
    special = {1: (a, 0), 2: (a - 1, 0), 3: (b, 0), 4: (b + 1, 0), 5: (a - 1, 1), 6: (b - 1, 1), 7: (b, 1), 8: (N // 2, mm), 9: (N // 2, mm + 1),
               10: (0, N), 11: (0, a), 12: (N // 2, 1), 13: (N // 2 - 1, mm), 14: (1, 1)}
    for v in range(V):
        if skip[v]:
            continue
        if v in special:
            n_p, n_m = special[v]
        else:
            n_m = int(rng.choice([0, 0, 0, 1, 1, 2, 3]))
            n_p = int(rng.integers(0, N - n_m + 1)) if rng.random() < 0.15 else int(rng.integers(max(1, N // 5), max(2, N - N // 5 - n_m)))
        perm = rng.permutation(N)
        P[v, perm[:n_p]] = 1
        M[v, perm[n_p:n_p + n_m]] = 1
    names = [("rec_%03d" % v) + "x" * int(rng.integers(0, 5)) for v in range(V)]
    enc = [x.encode() for x in names]
    off = np.zeros(V + 1, dtype=np.int64)
    np.cumsum([len(x) for x in enc], out=off[1:])
    case.update(y=y, P=P, M=M, skip=skip, names=names, blob=b"".join(enc), off=off, n_present=P.sum(axis=1).astype(np.int32),
                n_missing=M.sum(axis=1).astype(np.int32), samples=["s%03d" % ((7 * i) % N if N % 7 else i) for i in range(N)])
    return case
