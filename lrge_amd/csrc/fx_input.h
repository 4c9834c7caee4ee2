// fx_input.h -- the bytes of one input file as the device ingest reads them (host_fastx.inl, DESIGN sections 24 and 30): a buffer
// that is in memory already, or a descriptor that is read by range with pread.  No HIP and no library type: g++ compiles it alone
// (tools/stream_check.cpp).  A read gives all the bytes asked for or fails: a short read, a file that shrank and a descriptor that
// cannot be read by position are all `false`, and the caller reports an IO error -- never a partial result.
#pragma once
#include <fcntl.h>
#include <stdint.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

struct FxInput {
    const uint8_t *d = nullptr;
    uint64_t len = 0;
    int fd = -1;
    const char *path = nullptr;
    mutable uint64_t n_reads = 0, n_bytes = 0;  // read calls issued on the descriptor and the bytes they brought (lrge_hip_last_stream_stats)
    FxInput() = default;
    FxInput(const FxInput &) = delete;
    FxInput &operator=(const FxInput &) = delete;
    ~FxInput() { if (fd >= 0) close(fd); }
    // a regular file, opened for reading by range; its length by fstat
    bool open_path(const char *p) {
        struct stat st;
        path = p;
        if ((fd = open(p, O_RDONLY | O_CLOEXEC)) < 0 || fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) return false;
        len = (uint64_t)st.st_size;
        return true;
    }
    bool read(uint64_t off, uint64_t n, uint8_t *dst) const {
        if (off > len || n > len - off) return false;
        if (d) { if (n) memcpy(dst, d + off, (size_t)n); return true; }
        for (uint64_t got = 0; got < n;) {
            const ssize_t k = pread(fd, dst + got, (size_t)(n - got), (off_t)(off + got));
            ++n_reads;
            if (k <= 0) return false;
            got += (uint64_t)k; n_bytes += (uint64_t)k;
        }
        return true;
    }
    // the first / the last min(cap, len) bytes, for a sniff (*got: how many)
    bool head(uint8_t *dst, uint64_t cap, uint64_t *got) const { *got = cap < len ? cap : len; return read(0, *got, dst); }
    bool tail(uint8_t *dst, uint64_t cap, uint64_t *got) const { *got = cap < len ? cap : len; return read(len - *got, *got, dst); }
    // the last four bytes as a little-endian word: the ISIZE of a gzip file's last member, a first size for its text (0: a file below 18 bytes)
    bool gzip_isize(uint32_t *isize) const {
        uint8_t b[4];
        *isize = 0;
        if (len < 18) return true;
        if (!read(len - 4, 4, b)) return false;
        *isize = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
        return true;
    }
};
