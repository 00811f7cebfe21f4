"""Sample similarity (kinship) matrix from variant presence/absence: mirrors the reference's `similarity` script
(pyseer/similarity.py) with the accumulation K = G G^T done by libseerhip (csrc/sim_kernels.hip: bit-plane AND + popcount).

Same command line, same stderr progress lines, same TSV on stdout."""
import sys

import numpy as np

from . import __version__
from . import _route

block_size = 1000                      # pyseer/similarity.py:16 (sets the granularity of the 'Matrix size' progress lines)
_FLUSH_ROWS = 1 << 16                  # packed rows handed to the device per call
_SELECT_FLUSH_ROWS = 1 << 18           # the same for a cache's rows that are selected on the device: two chunks of the call's staging at 5000 samples


def get_options(argv=None):
    import argparse

    description = 'Calculate a similarity matrix using variant presence/absence information'
    parser = argparse.ArgumentParser(description=description, prog='similarity')
    parser.add_argument("samples", help="List of sample names to use")
    variant_group = parser.add_mutually_exclusive_group(required=True)
    variant_group.add_argument('--kmers', default=None, help='Kmers file')
    variant_group.add_argument('--vcf', default=None, help='VCF file. Will filter any non \'PASS\' sites')
    variant_group.add_argument('--pres', default=None, help='Presence/absence .Rtab matrix as produced by roary and piggy')
    variant_group.add_argument('--load-packed', default=None,
                               help='Packed k-mer cache (python -m pyseer_amd.pack) over the listed samples, or over a superset or another order of them: '
                                    'the cache alone is read, and K is printed by the device')
    parser.add_argument('--min-af', type=float, default=0.01, help='Minimum AF [Default: 0.01]')
    parser.add_argument('--max-af', type=float, default=0.99, help='Maximum AF [Default: 0.99]')
    parser.add_argument('--max-missing', type=float, default=0.05, help='Maximum missing (vcf/Rtab) [Default: 0.05]')
    parser.add_argument('--uncompressed', action='store_true', default=False,
                        help='Uncompressed kmers file [Default: gzipped]')
    parser.add_argument('--gpu', type=int, default=0, help='Device index [Default: 0]')
    parser.add_argument('--python-reader', action='store_true', default=False,
                        help='Parse k-mer, VCF and Rtab files with the Python reader instead of the native one')
    parser.add_argument('--device-reader', action='store_true', default=False,
                        help='Read the sample tokens of a --kmers file on the device (the native reader); ignored with --python-reader, --vcf and --pres')
    parser.add_argument('--device-inflate', action='store_true', default=False,
                        help='Decode the members of a BGZF (bgzip) --kmers file on the device as well; implies --device-reader and is ignored where that is')
    parser.add_argument('--version', action='version', version='%(prog)s ' + __version__)
    return parser.parse_args(argv)


class SimilarityAccumulator(object):
    """K = G G^T over packed presence rows, accumulated on the device; samples that carry a missing call in a kept variant
    come out as NaN rows/columns, as np.matmul over the reference's NaN-holding G gives (similarity.py:113)."""

    def __init__(self, n_samples, device=0):
        from .engine import Engine
        self.n = n_samples
        self.engine = Engine(n_samples, device=device)
        self.engine.sim_begin()
        self._pending = []
        self._rows = 0
        self._nan = np.zeros(n_samples, dtype=bool)

    def add_packed(self, bits):
        if bits.shape[0] == 0:
            return
        self._pending.append(bits)
        self._rows += bits.shape[0]
        if self._rows >= _FLUSH_ROWS:
            self.flush()

    def add_dense(self, k):
        """One variant as the reference's k vector (0/1, NaN = missing call)."""
        k = np.asarray(k, dtype=float)
        miss = np.isnan(k)
        self._nan |= miss
        from .packing import pack_variants
        self.add_packed(pack_variants(np.where(miss, 0.0, k)[None, :]))

    def flush(self):
        if self._pending:
            self.engine.sim_accumulate(np.ascontiguousarray(np.concatenate(self._pending, axis=0)))
        self._pending = []
        self._rows = 0

    def finish(self):
        self.flush()
        K = self.engine.sim_finish()
        if self._nan.any():
            K[self._nan, :] = np.nan
            K[:, self._nan] = np.nan
        return K


def similarity_matrix(p, var_type, infile, path, all_strains, sample_order, min_af, max_af, max_missing, uncompressed,
                      device=0, python_reader=False, progress=None, device_reader=False, device_inflate=None):
    """The loop of similarity.py:99-113 over PackedBlocks."""
    from .input import iter_packed_blocks, iter_packed_blocks_native, iter_packed_blocks_rtab_native, iter_packed_blocks_vcf_native
    acc = SimilarityAccumulator(len(p), device=device)
    if var_type == "kmers" and not python_reader:
        blocks = iter_packed_blocks_native(p, path, min_af, max_af, block_size, engine=(acc.engine if device_reader else None), inflate=device_inflate)
    elif var_type == "vcf" and not python_reader:       # the sample columns are tokenised on the accumulator's device (pyseer/similarity.py:86-88)
        blocks = iter_packed_blocks_vcf_native(p, path, acc.engine, min_af, max_af, max_missing, block_size, want_patterns=False)
    elif var_type == "Rtab" and not python_reader:      # the calls likewise (k_rtab_pack)
        blocks = iter_packed_blocks_rtab_native(p, path, acc.engine, min_af, max_af, max_missing, block_size, want_patterns=False)
    else:
        blocks = iter_packed_blocks(p, var_type, infile, all_strains, sample_order, min_af, max_af, max_missing,
                                    uncompressed, block_size, want_patterns=False)
    nblocks = 0
    for blk in blocks:
        st_arr = np.asarray(blk.status)
        # blocks of the native reader carry every parsed row (the association driver lets the engine apply the AF window); here only the kept
        # rows enter K = G G^T, as the reference's load_var_block drops the filtered ones (pyseer/input.py:693)
        acc.add_packed(blk.bits if (st_arr == 0).all() or blk.bits.shape[0] != st_arr.shape[0] else np.ascontiguousarray(blk.bits[st_arr == 0]))
        for st, k in zip(blk.status, blk.ks):
            if st == 2:
                acc.add_dense(k)
        nblocks += 1
        if progress is not None:
            progress(nblocks * block_size)
    if nblocks == 0 and progress is not None:
        progress(block_size)
    return acc.finish()


def progress_sizes(rows):
    """The sizes of the 'Matrix size' lines for a packed cache of `rows` stored rows: one per started `block_size` rows, as the text route
    says one per block of that many parsed lines; a cache without rows gets the one line an empty file gets."""
    return [block_size * i for i in range(1, max(1, -(-rows // block_size)) + 1)]


class _RowBatcher(object):
    """Stored blocks gathered into batches of `cap` rows for `sink`: every accumulation adds whole tiles of K, so it wants many rows at once
    (a cache's default block is 3000).  A block of at least `cap` rows that meets an empty batch is handed on as it lies in the mapping."""

    def __init__(self, row_bytes, cap, sink):
        self._rb, self._cap, self._sink = row_bytes, max(1, cap), sink
        self._buf, self._n = None, 0

    def add(self, bits):
        if self._n == 0 and bits.shape[0] >= self._cap:
            self._sink(bits)
            return
        while bits.shape[0]:
            if self._buf is None:
                self._buf = np.empty((self._cap, self._rb), dtype=np.uint8)
            k = min(self._cap - self._n, bits.shape[0])
            self._buf[self._n:self._n + k] = bits[:k]
            self._n += k
            bits = bits[k:]
            if self._n == self._cap:
                self.flush()

    def flush(self):
        if self._n:
            self._sink(self._buf[:self._n])
        self._n = 0


def _die(msg):
    sys.stderr.write(msg + "\n")
    sys.exit(1)


def main_packed(options, sample_list):
    """similarity --load-packed: K from a packed cache (python -m pyseer_amd.pack) over the listed samples, a superset or another order of
    them.  The cache's rows go up once: over the run's own list through sh_sim_accumulate, else restricted to the run's samples and
    accumulated on the device (sh_sim_accumulate_select); --min-af / --max-af are the context's filter over the run's samples; the matrix
    leaves the device as the text to print (sh_sim_text).  Everything that can refuse the run is decided before a context exists."""
    import pandas as pd
    from . import _abi
    from .input import announce_cache_select, check_packed_cache, open_packed_cache_rows
    path = options.load_packed
    if options.python_reader:
        _die("similarity: --python-reader reads text; it cannot be combined with --load-packed")
    seen = set()
    for s in sample_list:
        if s in seen:
            _die("similarity: sample %s is listed twice in %s" % (s, options.samples))
        seen.add(s)
    p = pd.Series(np.zeros(len(sample_list)), index=sample_list)
    try:
        stored, rb, total, rows = open_packed_cache_rows(path)
    except (IOError, OSError) as ex:
        _die("similarity: %s" % ex)
    have = set(stored)
    missing = [s for s in sample_list if s not in have]
    if missing:
        _die("similarity: packed cache %s lacks sample %s%s" % (path, missing[0], " and %d more" % (len(missing) - 1) if len(missing) > 1 else ""))
    try:
        selected = announce_cache_select(p, path, select="device")
        sample_map = check_packed_cache(p, path, select="device") if selected else None
    except (IOError, OSError, ValueError) as ex:
        _die("similarity: %s" % ex)
    sys.stderr.write("Reading in variants\n")
    from .engine import RowSelector, select_rows_host
    acc = SimilarityAccumulator(len(sample_list), device=options.gpu)
    acc.engine.set_af_filter(options.min_af, options.max_af)
    sel = None
    if not selected:
        feed = _RowBatcher(rb, _FLUSH_ROWS, acc.engine.sim_accumulate)
    elif _route.route("cache_select") == "host":
        feed = _RowBatcher(rb, _FLUSH_ROWS, lambda bits: acc.engine.sim_accumulate(select_rows_host(bits, len(stored), sample_map)[0]))
    else:
        sel = RowSelector(acc.engine, len(stored), sample_map)
        feed = _RowBatcher(rb, min(_SELECT_FLUSH_ROWS, max(total, 1)), sel.sim_accumulate)
    # stderr as the text route writes it: read_variant's message for a line nobody carries, 'Matrix size' after every block_size lines.  The
    # stored counts are the run's where the cache holds the run's samples and no others; over more samples they are not, and the counts
    # over the run's samples stay on the device: such a run does not say which lines nobody carries.
    sizes, said, done = progress_sizes(total), 0, 0
    say_empty = len(stored) == len(sample_list)

    def say_sizes(upto):
        nonlocal said
        for n in sizes[said:upto]:
            sys.stderr.write('Matrix size ' + str(n) + '\n')
        said = max(said, upto)
    for bits, empty in rows():
        feed.add(bits)
        for i, name in (empty if say_empty else ()):
            say_sizes((done + i) // block_size)
            sys.stderr.write("No observations of " + name + " in selected samples\n")
        done += bits.shape[0]
        say_sizes(done // block_size)
    say_sizes(len(sizes))
    feed.flush()
    if sel is not None:
        sel.close()
    sys.stderr.write("Calculating sample similarity\n")
    try:
        text = acc.engine.sim_text(sample_list)
    except _abi.SeerHipError as ex:
        if ex.code != _abi.SH_EINVAL:
            raise
        # (a matrix or names the device writer refuses: no real count gets here)
        pd.DataFrame(acc.finish(), index=p.index, columns=p.index).to_csv(sys.stdout, sep='\t')
        return
    out = getattr(sys.stdout, "buffer", None)
    if out is not None:
        sys.stdout.flush()
        out.write(text.data)
        out.flush()
    else:
        sys.stdout.write(text.tobytes().decode())


def main(argv=None):
    import pandas as pd
    from .input import open_variant_file

    options = get_options(argv)
    sample_list = []
    with open(options.samples, 'r') as sample_file:
        for sample in sample_file:
            sample_list.append(sample.rstrip())
    if options.load_packed:
        return main_packed(options, sample_list)
    p = pd.Series(np.zeros(len(sample_list)), index=sample_list)
    all_strains = set(p.index)
    sample_order = []
    infile = None
    path = None
    if options.kmers:
        var_type, path = "kmers", options.kmers
        if options.python_reader:
            infile, sample_order = open_variant_file("kmers", options.kmers, uncompressed=options.uncompressed)
    elif options.vcf:
        var_type, path = "vcf", options.vcf
        if options.python_reader:
            infile, sample_order = open_variant_file("vcf", options.vcf)
    else:
        var_type, path = "Rtab", options.pres
        if options.python_reader:
            infile, sample_order = open_variant_file("Rtab", options.pres)
    sys.stderr.write("Reading in variants\n")
    K = similarity_matrix(p, var_type, infile, path, all_strains, sample_order, options.min_af, options.max_af,
                          options.max_missing, options.uncompressed, device=options.gpu,
                          python_reader=options.python_reader,
                          device_reader=(options.device_reader or options.device_inflate or _route.route("kmer_dev", "0") == "1"
                                         or _route.route("kmer_inflate", "0") == "1"),
                          device_inflate=(True if options.device_inflate else None),
                          progress=lambda n: sys.stderr.write('Matrix size ' + str(n) + '\n'))
    sys.stderr.write("Calculating sample similarity\n")
    pd.DataFrame(K, index=p.index, columns=p.index).to_csv(sys.stdout, sep='\t')


if __name__ == "__main__":
    main()
