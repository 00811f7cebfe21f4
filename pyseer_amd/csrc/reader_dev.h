// reader_dev.h -- what the k-mer reader (reader.cpp, free of HIP) and the device half of its device route (kmer_api.inc) know of each other.
// A reader opened with hooks decodes into buffers the hooks allocate (pinned memory), says when a slab has arrived and when it is let go, and
// hands the framed lines of a call to `pack` instead of parsing their sample tokens itself.  Everything else -- containers, inflate, CRC, the
// newline index, names, the -2 accounting -- is the reader's, the same code as without hooks.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string>
#include "../../include/seerhip.h"

struct ShReaderLine {
    const char *p; size_t len;          // the line, without its newline
    const char *buf;                    // the slab buffer (as `alloc` returned it) the line lies in, or nullptr: in no slab (a line longer than the pad, reader=zlib)
};

// a BGZF member of a slab for `inflate`: its deflate body, and where its text goes (buf + pad + off); the hook fills in the last two
struct ShReaderMember {
    const uint8_t *cdata; uint32_t clen, isize; size_t off;
    int32_t status; uint32_t produced;     // 0 and isize: the text is there (the reader still checks its CRC-32)
};

struct ShReaderHooks {
    void *self = nullptr;
    char *(*alloc)(void *self, size_t bytes) = nullptr;                  // a slab buffer (called on the decoding thread)
    void (*release)(void *self, char *buf) = nullptr;
    // the bytes [from, to) of `buf` hold text now and will not change until slab_out; false: `err` says why
    bool (*slab_in)(void *self, const char *buf, size_t from, size_t to, std::string &err) = nullptr;
    void (*slab_out)(void *self, const char *buf) = nullptr;
    // rows and counts of `n` lines (bits is zeroed, row_bytes * 8 >= the sample count)
    bool (*pack)(void *self, const ShReaderLine *lines, int64_t n, uint8_t *bits, int64_t row_bytes, int32_t *counts, std::string &err) = nullptr;
    // optional (BGZF only): decode the `n` members of a slab into `buf` instead of the reader's decoding threads, once per slab, on the decoding
    // thread.  A member whose status, length or CRC-32 is wrong afterwards is decoded again by the reader; slab_in is then called with
    // [pad - carried tail, pad) first and once more for the range of every member decoded again.  false: the slab fails with `err`
    bool (*inflate)(void *self, char *buf, size_t pad, ShReaderMember *mem, int64_t n, std::string &err) = nullptr;
    void (*destroy)(void *self) = nullptr;                               // after the last buffer was released
};

// sh_reader_open with hooks (the reader owns `hooks.self` from here on, also when it returns nullptr)
sh_reader *sh_reader_open_hooked(const char *path, const char *const *sample_names, int n_samples, const ShReaderHooks &hooks);
void *sh_reader_hooks_self(sh_reader *r);                                // nullptr: opened without hooks
void sh_reader_set_error(const char *msg);                               // what sh_reader_error() answers on this thread
