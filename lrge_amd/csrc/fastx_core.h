// fastx_core.h -- the record scan of FASTA / FASTQ text, shared by the device (k_fastx.h, host_fastx.inl; hipcc) and the
// host twin (fastx_twin.cpp; g++): the per-byte predicates, the per-record rules and the host-side decisions between the
// passes.  The result must equal lrge::io::detail::parse_fastx (include/lrge_io.hpp) record for record; whatever these rules
// cannot prove is the verdict FX_UNPROVEN, and the caller takes the host parser.
//
// One predicate carries both formats: a byte is REMOVED when it is '\n', or a '\r' whose next byte is '\n' or the end of the
// text (the one CR the host's line reader strips).  A line is empty exactly when all its bytes are removed; the stripped
// length of any span is its size minus its removed bytes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FX_HD __host__ __device__ __forceinline__
#else
#define FX_HD static inline
#endif

#define FX_TILE 4096u          // text bytes per census tile on the device: 256 lanes x one 16-byte load
#define FX_EOT 0x100u          // the "byte" past the end of the text

enum { FX_FMT_EMPTY = 0, FX_FMT_FASTA = 1, FX_FMT_FASTQ = 2 };
// verdict bits (0: proven)
#define FX_UNPROVEN 1u
#define FX_TOO_MANY 2u

// one record: identifier bytes text[name_off, name_off + name_len), sequence text[seq_off, seq_off + seq_span) holding seq_len
// bases once the removed bytes are dropped (seq_span == seq_len: a single line, FASTQ always)
struct FxRec { uint64_t name_off, seq_off, seq_span; uint32_t name_len, seq_len; };

FX_HD bool fx_is_removed(uint32_t c, uint32_t next) { return c == '\n' || (c == '\r' && (next == '\n' || next == FX_EOT)); }
// a FASTA header is a local predicate: '>' at offset 0 (prev = '\n') or right behind a line feed
FX_HD bool fx_is_header(uint32_t c, uint32_t prev) { return c == '>' && prev == '\n'; }
FX_HD bool fx_is_space(uint32_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }

// masks of one group of 16 text bytes (little-endian words w[0..3]; `nvalid` of them lie inside the text; prev / next: the
// bytes around the group, '\n' before offset 0 and FX_EOT past the end): bit i is byte i
struct FxMasks { uint32_t lf, rem, hdr; };
FX_HD FxMasks fx_group_masks(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t prev, uint32_t next, uint32_t nvalid) {
    const uint32_t w[4] = {w0, w1, w2, w3};
    FxMasks m = {0, 0, 0};
    uint32_t p = prev;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t c = (w[i >> 2] >> ((i & 3) * 8)) & 0xFF;
        uint32_t nx = i < 15 ? (w[(i + 1) >> 2] >> (((i + 1) & 3) * 8)) & 0xFF : next;
        if (i + 1 >= nvalid) nx = i + 1 == nvalid && nvalid == 16 ? next : FX_EOT;
        if (i < nvalid) {
            m.lf |= (uint32_t)(c == '\n') << i;
            m.rem |= (uint32_t)fx_is_removed(c, nx) << i;
            m.hdr |= (uint32_t)fx_is_header(c, p) << i;
        }
        p = c;
    }
    return m;
}

// the identifier of a header whose bytes behind the marker are text[a, e): cut at the first whitespace byte
FX_HD uint64_t fx_name_len(const uint8_t *t, uint64_t a, uint64_t e) {
    uint64_t i = a;
    while (i < e && !fx_is_space(t[i])) ++i;
    return i - a;
}

// line j of the text as [*a, *e), its one trailing CR stripped.  ls[k], 0 <= k <= n_lf: where line k starts (ls[0] = 0,
// ls[k] = 1 + the offset of line feed k - 1); the line after the last line feed runs to the end of the text
FX_HD void fx_line(const uint8_t *t, uint64_t n, const uint64_t *ls, uint64_t n_lf, uint64_t j, uint64_t *a, uint64_t *e) {
    const uint64_t s = ls[j];
    uint64_t z = j < n_lf ? ls[j + 1] - 1 : n;
    if (z > s && t[z - 1] == '\r') --z;
    *a = s; *e = z;
}

// FASTQ record r of the strict form: lines l0 + 4r .. l0 + 4r + 3 (l0: the first non-empty line; n_lines: how many lines the
// host's reader would return).  Verdict bits; *rec is complete only when they are 0.
FX_HD uint32_t fx_fastq_record(const uint8_t *t, uint64_t n, const uint64_t *ls, uint64_t n_lf, uint64_t n_lines, uint64_t l0, uint64_t r, FxRec *rec) {
    const uint64_t j = l0 + 4 * r;
    if (j + 3 >= n_lines) return FX_UNPROVEN;                       // truncated record
    uint64_t a, e;
    fx_line(t, n, ls, n_lf, j, &a, &e);
    if (e == a || t[a] != '@') return FX_UNPROVEN;                  // an empty line between records, or no header here
    const uint64_t nl = fx_name_len(t, a + 1, e);
    rec->name_off = a + 1;
    fx_line(t, n, ls, n_lf, j + 2, &a, &e);
    if (e == a || t[a] != '+') return FX_UNPROVEN;
    fx_line(t, n, ls, n_lf, j + 1, &a, &e);
    rec->seq_off = a; rec->seq_span = e - a;
    if (nl >> 32) return FX_UNPROVEN;
    if ((e - a) >> 32) return FX_TOO_MANY;
    rec->name_len = (uint32_t)nl; rec->seq_len = (uint32_t)(e - a);
    return 0;
}

// FASTA record i: the header at hpos[i], hrem[i] removed bytes in front of it (modulo 2^32: only differences inside one
// record are used, and a record whose span reaches 2^32 is refused first); n_rem: the removed bytes of the whole text
FX_HD uint32_t fx_fasta_record(const uint8_t *t, uint64_t n, const uint64_t *hpos, const uint32_t *hrem, uint64_t n_hdr, uint64_t n_rem, uint64_t i, FxRec *rec) {
    const uint64_t h = hpos[i];
    uint64_t p = h + 1;
    while (p < n && t[p] != '\n') ++p;                              // the header's line feed, or the end of the text
    uint64_t e = p;
    if (t[e - 1] == '\r') --e;                                      // (e - 1 >= h, and t[h] is '>')
    const uint64_t nl = fx_name_len(t, h + 1, e);
    const uint32_t in_header = (uint32_t)(p < n) + (uint32_t)(e != p);
    const uint64_t a = p < n ? p + 1 : n, b = i + 1 < n_hdr ? hpos[i + 1] : n;
    const uint32_t rb = i + 1 < n_hdr ? hrem[i + 1] : (uint32_t)n_rem;
    rec->name_off = h + 1; rec->seq_off = a; rec->seq_span = b - a;
    if (nl >> 32) return FX_UNPROVEN;
    if ((b - a) >> 32) return (((b - a) - (n_rem < b - a ? n_rem : b - a)) >> 32) ? FX_TOO_MANY : FX_UNPROVEN;   // surely 2^32 bases : not counted here
    const uint32_t removed = rb - hrem[i] - in_header;
    rec->name_len = (uint32_t)nl; rec->seq_len = (uint32_t)(b - a) - removed;
    return 0;
}

// ---- host side, between the passes ----
// what the census pass knows of the whole text
struct FxCensus {
    uint64_t n_lf, n_rem, n_hdr;        // line feeds, removed bytes, FASTA headers
    uint64_t first, last;               // the first and last byte that is not removed (n: there is none)
    uint8_t head[4], at_first, tail;    // text[0..3] (0 past the end), text[first], text[n - 1]
};

// the format, from the first non-empty line (which starts at c.first: everything before it is removed); *verdict: 0 or FX_UNPROVEN
static inline int fx_format(uint64_t n, const FxCensus &c, uint32_t *verdict) {
    *verdict = 0;
    if (n == 0 || c.first >= n) return FX_FMT_EMPTY;                // no line with a byte in it: the host returns no record
    // what the host sniffs as BAM, CRAM or SAM never reaches its FASTA / FASTQ parser
    const uint8_t *h = c.head;
    if ((n >= 4 && h[0] == 'B' && h[1] == 'A' && h[2] == 'M' && h[3] == 1) || (n >= 4 && h[0] == 'C' && h[1] == 'R' && h[2] == 'A' && h[3] == 'M') ||
        (n >= 3 && h[0] == '@' && ((h[1] == 'H' && h[2] == 'D') || (h[1] == 'S' && h[2] == 'Q') || (h[1] == 'R' && h[2] == 'G')))) {
        *verdict = FX_UNPROVEN; return FX_FMT_EMPTY;
    }
    if (c.at_first == '>') return FX_FMT_FASTA;
    if (c.at_first == '@') return FX_FMT_FASTQ;
    *verdict = FX_UNPROVEN;
    return FX_FMT_EMPTY;
}

// the limits of the 32-bit scans: verdict bits before any table is built
static inline uint32_t fx_limits(int fmt, const FxCensus &c) {
    if (fmt == FX_FMT_FASTA) return c.n_hdr >> 32 ? FX_TOO_MANY : 0;
    if (fmt == FX_FMT_FASTQ) return c.n_lf >> 34 ? FX_TOO_MANY : c.n_lf >> 32 ? FX_UNPROVEN : 0;   // (2^32 lines and more: not proven here)
    return 0;
}

// FASTQ: l0 / l_last = the line feeds in front of c.first / c.last, i.e. the indices of the first and last non-empty line.
// Every line in between belongs to a group of four; the last group may end with an empty quality line.
static inline void fx_fastq_shape(uint64_t n, const FxCensus &c, uint64_t l0, uint64_t l_last, uint64_t *n_lines, uint64_t *n_rec) {
    *n_lines = c.n_lf + (uint64_t)(n > 0 && c.tail != '\n');
    *n_rec = (l_last - l0 + 4) / 4;
}
