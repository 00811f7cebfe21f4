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

struct ShReaderHooks {
    void *self = nullptr;
    char *(*alloc)(void *self, size_t bytes) = nullptr;                  // a slab buffer (called on the decoding thread)
    void (*release)(void *self, char *buf) = nullptr;
    // the bytes [from, to) of `buf` hold text now and will not change until slab_out; false: `err` says why
    bool (*slab_in)(void *self, const char *buf, size_t from, size_t to, std::string &err) = nullptr;
    void (*slab_out)(void *self, const char *buf) = nullptr;
    // rows and counts of `n` lines (bits is zeroed, row_bytes * 8 >= the sample count)
    bool (*pack)(void *self, const ShReaderLine *lines, int64_t n, uint8_t *bits, int64_t row_bytes, int32_t *counts, std::string &err) = nullptr;
    void (*destroy)(void *self) = nullptr;                               // after the last buffer was released
};

// sh_reader_open with hooks (the reader owns `hooks.self` from here on, also when it returns nullptr)
sh_reader *sh_reader_open_hooked(const char *path, const char *const *sample_names, int n_samples, const ShReaderHooks &hooks);
void *sh_reader_hooks_self(sh_reader *r);                                // nullptr: opened without hooks
void sh_reader_set_error(const char *msg);                               // what sh_reader_error() answers on this thread
