// inflate_core_check.cpp -- the host build of the DEFLATE core (pyseer_amd/csrc/inflate_dev.h) over a corpus file, as a program of its own
// for a sanitizer build:
//   python -c "import sys; sys.path.insert(0, 'tests'); import _inflate_corpus as c; print(c.write_corpus_file('/tmp/inflate.corpus'))"
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/inflate_core_check tools/inflate_core_check.cpp
//   /tmp/inflate_core_check /tmp/inflate.corpus
// Every member is decoded from a heap copy of exactly clen bytes into a heap buffer of exactly isize bytes, so a byte read or written
// outside either range is the sanitizer's to report.  A well-formed member must give status 0 and the expected bytes, a malformed one a
// status that is not 0.  The file format is written by tests/_inflate_corpus.py write_corpus_file.  Not a test of the suite; host only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../pyseer_amd/csrc/inflate_dev.h"

static bool get32(FILE *f, uint32_t *v)
{
    unsigned char b[4];
    if (fread(b, 1, 4, f) != 4) return false;
    *v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s corpus-file\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    char magic[6];
    uint32_t count = 0;
    if (!f || fread(magic, 1, 6, f) != 6 || memcmp(magic, "SHIC1\n", 6) != 0 || !get32(f, &count)) { fprintf(stderr, "%s: not a corpus file\n", argv[1]); return 2; }
    ShInfTables *t = new ShInfTables;
    int good = 0, bad = 0, failed = 0;
    int seen[16] = {0};
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t kind, clen, isize, nexp;
        if (!get32(f, &kind) || !get32(f, &clen) || !get32(f, &isize) || !get32(f, &nexp)) { fprintf(stderr, "member %u: the file ends\n", i); return 2; }
        uint8_t *c = (uint8_t *)malloc(clen ? clen : 1), *want = (uint8_t *)malloc(nexp ? nexp : 1), *out = (uint8_t *)malloc(isize ? isize : 1);
        if (fread(c, 1, clen, f) != clen || fread(want, 1, nexp, f) != nexp) { fprintf(stderr, "member %u: the file ends\n", i); return 2; }
        // (exact sizes: an empty range is a one-byte allocation that must stay untouched)
        uint8_t *cc = clen ? c : nullptr, *oo = isize ? out : nullptr;
        uint32_t produced = 0xffffffffu;
        const int st = shi_inflate(cc, clen, oo, isize, t, &produced, ShInfOne());
        seen[st & 15]++;
        if (produced > isize) { printf("member %u: produced %u of %u\n", i, produced, isize); ++failed; }
        if (kind == 0) {
            ++good;
            if (st != SHI_OK || produced != nexp || memcmp(out, want, nexp) != 0) { printf("member %u (well formed): status %d, %u of %u bytes\n", i, st, produced, nexp); ++failed; }
        } else {
            ++bad;
            if (st == SHI_OK) { printf("member %u (malformed): status 0\n", i); ++failed; }
        }
        free(c); free(want); free(out);
    }
    delete t;
    fclose(f);
    printf("%d well-formed and %d malformed members, %d failures; statuses seen:", good, bad, failed);
    for (int s = 0; s < 16; ++s) if (seen[s]) printf(" %d x%d", s, seen[s]);
    printf("\n");
    return failed ? 1 : 0;
}
