"""python -m pyseer_amd.pack samples.txt --kmers a.gz -o all.seerpack: a packed cache (input.py PackedCacheWriter) over ALL the listed isolates
of a k-mer file -- no phenotype, no AF filter, no GPU.  A later `python -m pyseer_amd ... --load-packed all.seerpack` over any subset or
order of those isolates (another phenotype column, one lineage, a covariate file that lacks some) has the cache's rows restricted to its
samples on the device instead of parsing the text again.

python -m pyseer_amd.pack samples.txt (--vcf F [--burden R] | --pres F) -o all.seercalls: the same for input with missing calls -- a call cache
(input.py CallCacheWriter) for `--load-calls`.  These two readers tokenise the calls on the device, so this form needs one (--gpu)."""
import sys

from . import __version__


def get_options(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description='Write a packed k-mer cache, or a call cache, over all listed samples', prog='pyseer_amd.pack')
    parser.add_argument("samples", help="List of sample names to store, one a line (as `similarity` takes it)")
    group = parser.add_mutually_exclusive_group(required=True)
    group.add_argument('--kmers', help='Kmers file: a packed k-mer cache is written (for --load-packed)')
    group.add_argument('--vcf', help='VCF or BCF file: a call cache is written (for --load-calls)')
    group.add_argument('--pres', help='Presence/absence .Rtab matrix: a call cache is written (for --load-calls)')
    parser.add_argument('--burden', help='With --vcf: the regions file; the cache then holds one folded variant per line of it')
    parser.add_argument('-o', '--output', required=True, help='The cache to write')
    parser.add_argument('--uncompressed', action='store_true', default=False, help='Uncompressed kmers file [Default: gzipped]')
    parser.add_argument('--block', type=int, default=3000,
                        help='Variants per stored block [Default: 3000]; a run never splits a stored block, so a run whose output depends on '
                             'where blocks end (--lmm with --lineage, --print-filtered) needs the --block_size it would use on the text')
    parser.add_argument('--gpu', type=int, default=0, help='GPU index for --vcf and --pres [Default: 0]')
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


def write_call_cache(samples, output, vcf=None, pres=None, burden=None, block=3000, device=0):
    """A call cache over `samples` from a VCF / BCF (burden: the regions file) or an Rtab, through the native readers -> the number of variants stored.
    What the readers say of a record ("Multiple alleles at ...") is stored with it, not written here."""
    import collections
    import pandas as pd
    from . import input as I
    from .engine import Engine
    p = pd.Series(0.0, index=samples)
    engine = Engine(len(samples), device=device)
    out = I.CallCacheWriter(output, samples, block)
    rows = 0
    try:
        if vcf is not None:
            regions = None
            if burden:
                regions = collections.deque([])
                I.load_burden(burden, regions)
                regions = list(regions)
            blocks = I.iter_call_blocks_vcf_native(p, vcf, engine, block, regions)
        else:
            blocks = I.iter_call_blocks_rtab_native(p, pres, engine, block)
        for cb in blocks:
            out.write(cb)
            rows += len(cb)
    except BaseException:
        out.abort()
        raise
    finally:
        engine.close()
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
    if options.burden and not options.vcf:
        sys.stderr.write("pyseer_amd.pack: --burden regions group the records of a --vcf\n")
        sys.exit(1)
    if options.kmers:
        if not options.uncompressed:
            from .input import check_kmers_gzipped
            check_kmers_gzipped([options.kmers])
        rows = write_cache(samples, options.kmers, options.output, options.block)
    else:
        from .input import RtabDuplicateSample
        try:
            rows = write_call_cache(samples, options.output, options.vcf, options.pres, options.burden, options.block, options.gpu)
        except RtabDuplicateSample as ex:
            sys.stderr.write("pyseer_amd.pack: %s: no call cache is written for such a table\n" % ex)
            sys.exit(1)
        except ValueError as ex:                               # (a malformed Rtab line: what the run itself says, and no cache)
            sys.stderr.write("pyseer_amd.pack: %s\n" % ex)
            sys.exit(1)
    sys.stderr.write("%d variants over %d samples written to %s\n" % (rows, len(samples), options.output))


if __name__ == "__main__":
    main()
