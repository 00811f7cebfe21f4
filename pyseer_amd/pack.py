"""python -m pyseer_amd.pack samples.txt --kmers a.gz -o all.seerpack: a packed cache (input.py PackedCacheWriter) over ALL the listed isolates
of a k-mer file -- no phenotype, no AF filter, no GPU.  A later `python -m pyseer_amd ... --load-packed all.seerpack` over any subset or
order of those isolates (another phenotype column, one lineage, a covariate file that lacks some) has the cache's rows restricted to its
samples on the device instead of parsing the text again."""
import sys

from . import __version__


def get_options(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description='Write a packed k-mer cache over all listed samples', prog='pyseer_amd.pack')
    parser.add_argument("samples", help="List of sample names to store, one a line (as `similarity` takes it)")
    parser.add_argument('--kmers', required=True, help='Kmers file')
    parser.add_argument('-o', '--output', required=True, help='The cache to write (for --load-packed)')
    parser.add_argument('--uncompressed', action='store_true', default=False, help='Uncompressed kmers file [Default: gzipped]')
    parser.add_argument('--block', type=int, default=3000,
                        help='Variants per stored block [Default: 3000]; a run never splits a stored block, so a run whose output depends on '
                             'where blocks end (--lmm with --lineage) needs the --block_size it would use on the text')
    parser.add_argument('--version', action='version', version='%(prog)s ' + __version__)
    return parser.parse_args(argv)


def write_cache(samples, kmers, output, block=3000):
    """-> the number of variants stored"""
    from .input import NativeKmerReader, PackedCacheWriter
    reader = NativeKmerReader(kmers, samples, block)
    out = PackedCacheWriter(output, samples)
    rows = 0
    try:
        for bits, counts, blob, off in reader.raw_blocks():
            out.write_block(blob, off, counts, bits)
            rows += int(counts.shape[0])
    except BaseException:
        out.abort()
        raise
    finally:
        reader.close()
    out.close()
    return rows


def main(argv=None):
    options = get_options(argv)
    with open(options.samples, 'r') as sample_file:
        samples = [sample.rstrip() for sample in sample_file]
    seen = set()
    for s in samples:
        if s in seen:
            sys.stderr.write("pyseer_amd.pack: sample %s is listed twice in %s\n" % (s, options.samples))
            sys.exit(1)
        seen.add(s)
    if not samples:
        sys.stderr.write("pyseer_amd.pack: %s lists no samples\n" % options.samples)
        sys.exit(1)
    if options.block < 1:
        sys.stderr.write("pyseer_amd.pack: --block must be at least 1\n")
        sys.exit(1)
    if not options.uncompressed:
        from .input import check_kmers_gzipped
        check_kmers_gzipped([options.kmers])
    rows = write_cache(samples, options.kmers, options.output, options.block)
    sys.stderr.write("%d variants over %d samples written to %s\n" % (rows, len(samples), options.output))


if __name__ == "__main__":
    main()
