"""python -m pyseer_amd.count_patterns PATTERNS [--alpha A] [--threshold]

The reference's scripts/count_patterns.py for a pattern file that exists already (--output-patterns): the number of distinct 25-byte lines
and the Bonferroni threshold alpha / count, printed as the reference prints them.  Host only: numpy takes the distinct lines, no `sort`
process.  A run that has not happened yet gets the same two lines from `--count-patterns FILE`, counted on the device while it goes.
"""
import argparse
import sys
from decimal import Decimal

import numpy as np

LINE = 25                                      # base64 of 16 digest bytes (24 characters) and the newline


def threshold_text(alpha, count):
    """'%.2E' % Decimal(alpha / count) as the reference formats it; 'NA' for an empty set."""
    return 'NA' if count <= 0 else '%.2E' % Decimal(alpha / float(count))


def result_text(count, alpha=0.05):
    """The two lines the reference script prints."""
    return "Patterns:\t%d\nThreshold:\t%s\n" % (count, threshold_text(alpha, count))


_B64 = np.full(256, 0, dtype=np.uint32)
_B64[np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/", dtype=np.uint8)] = np.arange(64, dtype=np.uint32)


def digests_of_lines(text):
    """(n, 16) uint8: the digest bytes of n pattern lines (bytes-like, 25 n bytes) -- the keys a PatternSet takes for host-made patterns."""
    a = np.frombuffer(text, dtype=np.uint8)
    if a.size % LINE:
        raise ValueError("pattern text is not a whole number of %d-byte lines" % LINE)
    v = _B64[a.reshape(-1, LINE)[:, :24]].reshape(-1, 6, 4)             # (the two '=' decode as 0: the 18th byte is dropped below)
    x = (v[:, :, 0] << 18) | (v[:, :, 1] << 12) | (v[:, :, 2] << 6) | v[:, :, 3]
    out = np.empty((x.shape[0], 6, 3), dtype=np.uint8)
    out[:, :, 0] = x >> 16; out[:, :, 1] = (x >> 8) & 0xFF; out[:, :, 2] = x & 0xFF
    return np.ascontiguousarray(out.reshape(-1, 18)[:, :16])


def count_file(path):
    """Distinct lines of a pattern file (what `LC_ALL=C sort -u | wc -l` gives)."""
    with open(path, 'rb') as fh:
        data = fh.read()
    if not data:
        return 0
    if len(data) % LINE == 0 and data[LINE - 1::LINE] == b"\n" * (len(data) // LINE):
        lines = np.frombuffer(data, dtype=np.dtype((np.void, LINE)))
        return int(np.unique(lines).shape[0])
    return len(set(data.split(b"\n")[:-1] if data.endswith(b"\n") else data.split(b"\n")))   # (a file of another make: any lines)


def get_options(argv=None):
    parser = argparse.ArgumentParser(prog='python -m pyseer_amd.count_patterns', description='Calculate p-value threshold using Bonferroni correction')
    parser.add_argument('patterns', help='File of patterns from pyseer')
    parser.add_argument('--threshold', default=False, action='store_true', help='Only print p-value threshold')
    parser.add_argument('--alpha', default=0.05, type=float, help='Family-wise error rate')
    parser.add_argument('--cores', default=1, help='Accepted for compatibility; ignored')
    parser.add_argument('--memory', default=1024, help='Accepted for compatibility; ignored')
    parser.add_argument('--temp', default='/tmp', help='Accepted for compatibility; ignored')
    return parser.parse_args(argv)


def main(argv=None):
    options = get_options(argv)
    n = count_file(options.patterns)
    if options.threshold:
        sys.stdout.write(threshold_text(options.alpha, n) + "\n")
    else:
        sys.stdout.write(result_text(n, options.alpha))


if __name__ == "__main__":
    main()
