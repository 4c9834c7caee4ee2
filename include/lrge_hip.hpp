// lrge_hip.hpp -- C++ host-side mirror of liblrge's operator interface on top of the C ABI
// (include/lrge_hip.h).  Header-only.  The reference is Rust (no Rust toolchain in this image), so the
// compiled-language host side is C++; names, defaults and error behaviour follow the reference:
//   trait Estimate / EstimateResult        liblrge/src/estimate.rs:8-78
//   twoset::Builder / TwoSetStrategy       liblrge/src/twoset/builder.rs:22-185, twoset.rs:75-201,587-606
//   ava::Builder / AvaStrategy             liblrge/src/ava/builder.rs:19-153, ava.rs:71-161,369-382
//   LrgeError                              liblrge/src/error.rs:6-33
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <numeric>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <unordered_set>
#include <utility>
#include <vector>

#include "lrge_hip.h"
#include "lrge_rand.hpp"

namespace lrge {

struct LrgeError : std::runtime_error {
    int code;   // LRGE_ERR_*
    LrgeError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

constexpr float LOWER_QUANTILE = 0.15f, UPPER_QUANTILE = 0.65f;   // estimate.rs:40-46
enum class Platform { Nanopore, PacBio };                          // lib.rs:128-145

struct EstimateResult {   // estimate.rs:8-17
    std::optional<float> lower, estimate, upper;
    uint32_t no_mapping_count = 0;
};

struct Reads {            // parsed records: what io::iter_records hands to the strategies
    std::vector<std::string> names, seqs;
};

// trait Estimate (estimate.rs:21-78)
class Estimate {
public:
    virtual ~Estimate() = default;
    virtual std::pair<std::vector<float>, uint32_t> generate_estimates() = 0;
    EstimateResult estimate(bool finite, std::optional<float> lower_quant, std::optional<float> upper_quant) {
        auto [est, no_map] = generate_estimates();
        float out[3]; int ok[3];
        int rc = lrge_hip_median(est.data(), est.size(), finite ? 1 : 0, lower_quant ? 1 : 0, lower_quant.value_or(0.f),
                                 upper_quant ? 1 : 0, upper_quant.value_or(0.f), out, ok);
        if (rc) throw LrgeError(rc, "invalid quantile arguments");
        EstimateResult r;
        if (ok[0]) r.lower = out[0];
        if (ok[1]) r.estimate = out[1];
        if (ok[2]) r.upper = out[2];
        r.no_mapping_count = no_map;
        return r;
    }
};

namespace detail {
struct Ctx {
    lrge_hip_ctx *h = nullptr;
    explicit Ctx(int device) {
        int rc = lrge_hip_ctx_create(device, &h);
        if (rc) throw LrgeError(rc, std::string("device: ") + lrge_hip_last_error(nullptr));
    }
    ~Ctx() { lrge_hip_ctx_destroy(h); }
    void check(int rc) const { if (rc) throw LrgeError(rc, lrge_hip_last_error(h)); }
};
}  // namespace detail

// The records of one FASTA / FASTQ file (or, with | LRGE_GPU_INGEST_BAM / LRGE_GPU_INGEST_SAM, one unaligned BAM / SAM) parsed on the device;
// | LRGE_GPU_INGEST_WINDOWED: FASTA / FASTQ text above option INGEST_WINDOW_BYTES passes through in windows and only the bases stay;
// | LRGE_GPU_INGEST_WINDOWED_ALN beside it and the format's flag: unaligned BAM (its bases kept packed) and SAM as well;
// | LRGE_GPU_INFLATE_BZIP2, | LRGE_GPU_INFLATE_ZSTD, | LRGE_GPU_INFLATE_XZ: bzip2, Zstandard and xz input decompressed on the device too (Zstandard text is never windowed without the next flag)
// | LRGE_GPU_INGEST_WINDOWED_ZSTD (opt-in) beside LRGE_GPU_INFLATE_ZSTD: Zstandard text passes through the windows too, and census / open_selected / census_map / open_mapped take it;
// | LRGE_GPU_INGEST_SELECT_ALN (opt-in) beside LRGE_GPU_INGEST_BAM: census / open_selected / census_map / open_mapped take unaligned BAM too;
// | LRGE_GPU_INGEST_SELECT_SAM (opt-in) beside LRGE_GPU_INGEST_SAM: ... and unaligned SAM;
// | LRGE_GPU_INGEST_SELECT_CRAM (opt-in) beside LRGE_GPU_INGEST_CRAM: ... and unaligned CRAM;
// | LRGE_GPU_INGEST_STREAM (opt-in): open / census / open_selected / census_map read plain, BGZF and gzip files in pinned pieces of option INGEST_STREAM_BYTES instead of whole (open needs LRGE_GPU_INGEST_WINDOWED beside it);
// | LRGE_GPU_INGEST_CRAM (opt-in, implied by nothing): unaligned CRAM, walked on the host, its base blocks decoded on the device (the flags pass through as given)
// (lrge_hip_reads_open, io.rs:154-184): identifiers and lengths on
// the host, the bases resident in HBM as text.  Owns its context; the strategies built on it run in that context and take
// their read sets with lrge_hip_seqset_from_reads.  open() gives nullptr for input the device does not prove (and for a file
// it cannot read): the caller parses the file into a Reads with io::iter_records, which reports whatever is wrong with it.
struct DeviceReads {
    std::shared_ptr<detail::Ctx> ctx;
    lrge_hip_reads *h = nullptr;
    std::vector<std::string> names;
    std::vector<uint32_t> lens;
    uint64_t window_stats[4] = {0, 0, 0, 0};   // lrge_hip_reads_window_stats: windows flushed (0: resident), bytes in the store (BAM: packed bases), largest window, bytes carried
    DeviceReads() = default;
    DeviceReads(const DeviceReads &) = delete;
    DeviceReads &operator=(const DeviceReads &) = delete;
    ~DeviceReads() { lrge_hip_reads_free(h); }
    static std::unique_ptr<DeviceReads> open(const std::string &path, int flags = LRGE_GPU_INFLATE_BGZF | LRGE_GPU_INFLATE_GZIP, int device = 0) {
        auto r = std::make_unique<DeviceReads>();
        r->ctx = std::make_shared<detail::Ctx>(device);
        const int rc = lrge_hip_reads_open(r->ctx->h, path.c_str(), flags, &r->h);
        if (rc == LRGE_ERR_UNPROVEN || rc == LRGE_ERR_IO) return nullptr;
        r->ctx->check(rc);
        r->tables();
        return r;
    }
    // The device ingest of a sample.  census: the count pass (lrge_hip_reads_census, io.rs:140-145) -- out =
    // {records, sequence bases, text bytes, windows}; false for input the device does not prove or cannot read, as open()'s
    // nullptr.  `ctx`: a context to run in (none: one is made on `device`)
    static bool census(const std::string &path, int flags, int device, uint64_t out[4], std::shared_ptr<detail::Ctx> ctx = nullptr) {
        if (!ctx) ctx = std::make_shared<detail::Ctx>(device);
        const int rc = lrge_hip_reads_census(ctx->h, path.c_str(), flags, out);
        if (rc == LRGE_ERR_UNPROVEN || rc == LRGE_ERR_IO) return false;
        ctx->check(rc);
        return true;
    }
    // open_selected: the pass that keeps records sel (strictly ascending ordinals; lrge_hip_reads_open_selected, twoset.rs:122-201):
    // a DeviceReads of sel.size() reads in file order, select_stats filled; nullptr as open()
    static std::unique_ptr<DeviceReads> open_selected(const std::string &path, int flags, const std::vector<uint32_t> &sel, int device = 0,
                                                      std::shared_ptr<detail::Ctx> ctx = nullptr) {
        auto r = std::make_unique<DeviceReads>();
        r->ctx = ctx ? ctx : std::make_shared<detail::Ctx>(device);
        const int rc = lrge_hip_reads_open_selected(r->ctx->h, path.c_str(), flags, sel.data(), (uint32_t)sel.size(), &r->h);
        if (rc == LRGE_ERR_UNPROVEN || rc == LRGE_ERR_IO) return nullptr;
        r->ctx->check(rc);
        r->ctx->check(lrge_hip_reads_select_stats(r->h, r->select_stats));
        r->tables();
        return r;
    }
    uint64_t select_stats[4] = {0, 0, 0, 0};   // lrge_hip_reads_select_stats: records seen, kept, sequence bases seen, kept (open_selected)
    // The same two passes with a seek map.  census_map: census that also leaves the map (lrge_hip_reads_census_map;
    // free it with lrge_hip_read_map_free).  open_mapped: open_selected that brings only the runs of the map that hold records sel
    // (lrge_hip_reads_open_mapped), seek_stats filled; nullptr as open(), *rc_out (may be null) the call's code
    static bool census_map(const std::string &path, int flags, int device, uint64_t out[4], lrge_hip_read_map **map, std::shared_ptr<detail::Ctx> ctx = nullptr) {
        if (!ctx) ctx = std::make_shared<detail::Ctx>(device);
        const int rc = lrge_hip_reads_census_map(ctx->h, path.c_str(), flags, out, map);
        if (rc == LRGE_ERR_UNPROVEN || rc == LRGE_ERR_IO) return false;
        ctx->check(rc);
        return true;
    }
    static std::unique_ptr<DeviceReads> open_mapped(const std::string &path, int flags, const lrge_hip_read_map *map, const std::vector<uint32_t> &sel, int device = 0,
                                                    std::shared_ptr<detail::Ctx> ctx = nullptr, int *rc_out = nullptr) {
        auto r = std::make_unique<DeviceReads>();
        r->ctx = ctx ? ctx : std::make_shared<detail::Ctx>(device);
        const int rc = lrge_hip_reads_open_mapped(r->ctx->h, path.c_str(), flags, map, sel.data(), (uint32_t)sel.size(), &r->h);
        if (rc_out) *rc_out = rc;
        if (rc == LRGE_ERR_UNPROVEN || rc == LRGE_ERR_IO) return nullptr;
        r->ctx->check(rc);
        r->ctx->check(lrge_hip_reads_select_stats(r->h, r->select_stats));
        r->ctx->check(lrge_hip_reads_seek_stats(r->h, r->seek_stats));
        r->tables();
        return r;
    }
    uint64_t zstd_stats[4] = {0, 0, 0, 0};     // lrge_hip_reads_zstd_stats: rounds, largest history, largest work text, bytes of history moved (zeros: the call did not slide)
    uint64_t seek_stats[4] = {0, 0, 0, 0};     // lrge_hip_reads_seek_stats: runs, text bytes brought, file bytes read, BGZF blocks decoded (open_mapped)
private:
    void tables() {
        ctx->check(lrge_hip_reads_window_stats(h, window_stats));
        ctx->check(lrge_hip_reads_zstd_stats(h, zstd_stats));
        const uint64_t n = lrge_hip_reads_count(h);
        std::vector<uint64_t> off(n + 1);
        std::string blob(lrge_hip_reads_name_bytes(h), '\0');
        lens.resize(n);
        ctx->check(lrge_hip_reads_table(h, lens.data(), off.data(), blob.empty() ? nullptr : &blob[0]));
        names.reserve(n);
        for (uint64_t i = 0; i < n; ++i) names.emplace_back(blob, off[i], off[i + 1] - off[i]);
    }
};

// The input of a strategy that takes only its sample through the device: the census gives n, the strategy
// applies the reference's checks to it and draws its indices exactly as on a DeviceReads, and only the drawn reads are opened
// (DeviceReads::open_selected).  The estimate is bit for bit that of the same run through DeviceReads::open.
struct SampledSource {
    std::string path;
    int flags = LRGE_GPU_INFLATE_BGZF | LRGE_GPU_INFLATE_GZIP, device = 0;
    std::shared_ptr<detail::Ctx> ctx;           // made by census(); the strategy runs in it
    uint64_t counts[4] = {0, 0, 0, 0};          // the census: records, sequence bases, text bytes, windows
    bool counted = false;
    bool seek = false;                          // the census keeps a seek map, and open() brings only the runs that hold drawn reads
    std::shared_ptr<lrge_hip_read_map> map;     // the census's, when `seek`
    // the count pass, once; false: the device does not prove this input -- take DeviceReads::open, then the host readers
    bool census() {
        if (counted) return true;
        if (!ctx) ctx = std::make_shared<detail::Ctx>(device);
        if (!seek) return counted = DeviceReads::census(path, flags, device, counts, ctx);
        lrge_hip_read_map *m = nullptr;
        counted = DeviceReads::census_map(path, flags, device, counts, &m, ctx);
        map.reset(m, lrge_hip_read_map_free);
        return counted;
    }
    // the drawn ordinals (any order) opened in file order; the pass must see the census's records
    std::shared_ptr<DeviceReads> open(const std::vector<uint32_t> &idx, std::vector<uint32_t> *ascending) {
        *ascending = idx;
        std::sort(ascending->begin(), ascending->end());
        std::shared_ptr<DeviceReads> r;
        int rc = LRGE_ERR_UNPROVEN;
        if (seek && map) r = DeviceReads::open_mapped(path, flags, map.get(), *ascending, device, ctx, &rc);
        // (a map that does not fit the input: the pass of the whole file decides; any other refusal stands)
        if (!r && rc == LRGE_ERR_UNPROVEN) r = DeviceReads::open_selected(path, flags, *ascending, device, ctx);
        if (!r) throw LrgeError(LRGE_ERR_UNPROVEN, std::string("sampled ingest: ") + lrge_hip_last_error(ctx->h));
        if (r->select_stats[0] != counts[0])
            throw LrgeError(LRGE_ERR_IO, "IO error: the input changed between the count and the selection (" + std::to_string(counts[0]) + " records, then " + std::to_string(r->select_stats[0]) + ")");
        return r;
    }
};

namespace detail {
struct SeqSet {
    lrge_hip_seqset *h = nullptr;
    std::vector<uint32_t> lens;
    // reads idx of a DeviceReads (dev != nullptr), or the given host sequences
    SeqSet(const Ctx &c, const DeviceReads *dev, const std::vector<size_t> &idx, const std::vector<const std::string *> &seqs, const std::vector<uint32_t> &ranks) {
        if (!dev) { upload(c, seqs, ranks); return; }
        std::vector<uint32_t> ix(idx.begin(), idx.end());
        for (uint32_t i : ix) lens.push_back(dev->lens[i]);
        c.check(lrge_hip_seqset_from_reads(c.h, dev->h, ix.data(), (uint32_t)ix.size(), ranks.data(), &h));
    }
    SeqSet(const Ctx &c, const std::vector<const std::string *> &seqs, const std::vector<uint32_t> &ranks) { upload(c, seqs, ranks); }
    void upload(const Ctx &c, const std::vector<const std::string *> &seqs, const std::vector<uint32_t> &ranks) {
        std::vector<uint64_t> off(seqs.size() + 1, 0);
        for (size_t i = 0; i < seqs.size(); ++i) { off[i + 1] = off[i] + seqs[i]->size(); lens.push_back((uint32_t)seqs[i]->size()); }
        std::string cat; cat.reserve(off.back());
        for (auto *s : seqs) cat += *s;
        c.check(lrge_hip_seqset_upload(c.h, cat.data(), off.data(), (uint32_t)seqs.size(), ranks.data(), &h));
    }
    ~SeqSet() { lrge_hip_seqset_free(h); }
};
struct Index {
    lrge_hip_index *h = nullptr;
    Index(const Ctx &c, const SeqSet &s, int preset) { c.check(lrge_hip_index_build(c.h, s.h, preset, &h)); }
    ~Index() { lrge_hip_index_free(h); }
};
// strcmp ranks over the union of the given name lists (equal names share a rank)
inline std::vector<std::vector<uint32_t>> name_ranks(const std::vector<std::vector<const std::string *>> &lists) {
    std::vector<std::pair<const std::string *, std::pair<size_t, size_t>>> all;
    for (size_t l = 0; l < lists.size(); ++l) for (size_t i = 0; i < lists[l].size(); ++i) all.push_back({lists[l][i], {l, i}});
    std::sort(all.begin(), all.end(), [](auto &a, auto &b) { return *a.first < *b.first; });   // byte-wise, like strcmp
    std::vector<std::vector<uint32_t>> out(lists.size());
    for (size_t l = 0; l < lists.size(); ++l) out[l].resize(lists[l].size());
    uint32_t r = 0;
    for (size_t j = 0; j < all.size(); ++j) {
        if (j && *all[j].first != *all[j - 1].first) r = (uint32_t)j;
        out[all[j].second.first][all[j].second.second] = r;
    }
    return out;
}
// the same ranks computed on the device (lrge_hip_name_ranks): the names of all lists back to back, ranked as
// one selection and split again.  A name the device form does not take throws LrgeError with code LRGE_ERR_UNPROVEN.
inline std::vector<std::vector<uint32_t>> name_ranks_device(Ctx &c, const std::vector<std::vector<const std::string *>> &lists) {
    std::string blob;
    std::vector<uint64_t> off(1, 0);
    for (auto &l : lists) for (auto *s : l) { blob += *s; off.push_back(blob.size()); }
    const uint64_t n = off.size() - 1;
    std::vector<uint32_t> ranks(n ? n : 1);
    c.check(lrge_hip_name_ranks(c.h, blob.data(), off.data(), n, nullptr, n, ranks.data(), nullptr));
    std::vector<std::vector<uint32_t>> out(lists.size());
    size_t k = 0;
    for (size_t l = 0; l < lists.size(); ++l) { out[l].assign(ranks.begin() + (std::ptrdiff_t)k, ranks.begin() + (std::ptrdiff_t)(k + lists[l].size())); k += lists[l].size(); }
    return out;
}
// what a strategy calls: the device form when asked for, the host sort when not or when the device form hands the names back
// (LRGE_ERR_UNPROVEN only); note (may be empty) hears which of the two ran
inline std::vector<std::vector<uint32_t>> name_ranks_by(Ctx &c, bool on_device, const std::function<void(bool)> &note,
                                                        const std::vector<std::vector<const std::string *>> &lists) {
    if (on_device) {
        try {
            auto r = name_ranks_device(c, lists);
            if (note) note(true);
            return r;
        } catch (const LrgeError &e) {
            if (e.code != LRGE_ERR_UNPROVEN) throw;
        }
        if (note) note(false);
    }
    return name_ranks(lists);
}
// lib.rs:189-204: StdRng::seed_from_u64 + rand::seq::index::sample, restated in lrge_rand.hpp
using ::lrge::unique_random_set;
}  // namespace detail

// BGZF input decompressed on the device (lrge_hip_bgzf_inflate), as the inflater hook of io::iter_records(path, cb, hook)
// in lrge_io.hpp: false (the host path decompresses) for input that is not BGZF or holds a block the device rejects; a
// device failure throws.  The hook owns a context on `device` for as long as it lives.
namespace detail {
inline bool is_zstd(const std::string &raw) { return raw.size() >= 4 && (unsigned char)raw[0] == 0x28 && (unsigned char)raw[1] == 0xb5 && (unsigned char)raw[2] == 0x2f && (unsigned char)raw[3] == 0xfd; }
inline bool is_xz(const std::string &raw) { return raw.size() >= 6 && std::memcmp(raw.data(), "\xfd" "7zXZ\0", 6) == 0; }
inline bool is_bzip2(const std::string &raw) { return raw.size() >= 2 && raw[0] == 0x42 && raw[1] == 0x5a; }   // (lrge_io.hpp: detect_compression_format)
inline bool bgzf_inflate_with(Ctx &ctx, const std::string &raw, std::string &out) {
    uint64_t total = 0;
    if (lrge_hip_bgzf_scan(raw.data(), raw.size(), nullptr, &total) != LRGE_OK) return false;
    out.resize((size_t)total);
    const int rc = lrge_hip_bgzf_inflate(ctx.h, raw.data(), raw.size(), &out[0], total);
    if (rc == LRGE_ERR_PARSE) { out.clear(); return false; }
    ctx.check(rc);
    return true;
}
// a round decoder's C entry (lrge_hip_gzip_inflate, _bzip2_, _zstd_, _xz_) into `out`: false, with `out` empty, for the return
// codes in `host` (the host path decompresses, with its messages); any other failure throws
template <class Stats>
inline bool stream_inflate_with(Ctx &ctx, int (*entry)(lrge_hip_ctx *, const void *, uint64_t, int (*)(void *, const void *, uint64_t), void *, Stats *),
                                std::initializer_list<int> host, const std::string &raw, std::string &out) {
    out.clear();
    const int rc = entry(ctx.h, raw.data(), raw.size(), [](void *u, const void *b, uint64_t n) {
        static_cast<std::string *>(u)->append(static_cast<const char *>(b), (size_t)n);
        return 0;
    }, &out, nullptr);
    if (std::find(host.begin(), host.end(), rc) != host.end()) { out.clear(); return false; }
    ctx.check(rc);
    return true;
}
}  // namespace detail

inline std::function<bool(const std::string &, std::string &)> bgzf_inflater(int device) {
    auto ctx = std::make_shared<detail::Ctx>(device);
    return [ctx](const std::string &raw, std::string &out) -> bool { return detail::bgzf_inflate_with(*ctx, raw, out); };
}

// Every gzip input decompressed on the device: BGZF by k_inflate (as bgzf_inflater), any other gzip by the speculative
// decode (lrge_hip_gzip_inflate).  False (the host path decompresses, with its messages) for input the device cannot prove:
// damaged data, trailing bytes, a chunk beyond its slot; a device failure throws.
inline std::function<bool(const std::string &, std::string &)> gzip_inflater(int device) {
    auto ctx = std::make_shared<detail::Ctx>(device);            // one context for both device paths
    return [ctx](const std::string &raw, std::string &out) -> bool {
        if (detail::is_bzip2(raw) || detail::is_zstd(raw) || detail::is_xz(raw)) return false;
        if (lrge_hip_bgzf_scan(raw.data(), raw.size(), nullptr, nullptr) == LRGE_OK) return detail::bgzf_inflate_with(*ctx, raw, out);
        return detail::stream_inflate_with(*ctx, lrge_hip_gzip_inflate, {LRGE_ERR_PARSE, LRGE_ERR_TOO_MANY}, raw, out);
    };
}

// bzip2 input decompressed on the device (lrge_hip_bzip2_inflate); gzip input goes to `gzip` when one is given (gzip_inflater,
// bgzf_inflater).  False (the host path decompresses, with its messages) for input the device does not accept; a device
// failure throws.
inline std::function<bool(const std::string &, std::string &)> bzip2_inflater(int device, std::function<bool(const std::string &, std::string &)> gzip = nullptr) {
    auto ctx = std::make_shared<detail::Ctx>(device);
    return [ctx, gzip](const std::string &raw, std::string &out) -> bool {
        if (!detail::is_bzip2(raw)) return gzip ? gzip(raw, out) : false;
        return detail::stream_inflate_with(*ctx, lrge_hip_bzip2_inflate, {LRGE_ERR_PARSE}, raw, out);
    };
}

// Zstandard input decompressed on the device (lrge_hip_zstd_inflate); every other input goes to `other` when one is given
// (bzip2_inflater, gzip_inflater, bgzf_inflater).  False (the host path decompresses, with its messages) for input the device
// does not accept or that does not fit its budget; a device failure throws.
inline std::function<bool(const std::string &, std::string &)> zstd_inflater(int device, std::function<bool(const std::string &, std::string &)> other = nullptr) {
    auto ctx = std::make_shared<detail::Ctx>(device);
    return [ctx, other](const std::string &raw, std::string &out) -> bool {
        if (!detail::is_zstd(raw)) return other ? other(raw, out) : false;
        return detail::stream_inflate_with(*ctx, lrge_hip_zstd_inflate, {LRGE_ERR_PARSE, LRGE_ERR_TOO_MANY}, raw, out);
    };
}

// xz input decompressed on the device (lrge_hip_xz_inflate); every other input goes to `other` when one is given (zstd_inflater,
// bzip2_inflater, gzip_inflater, bgzf_inflater).  False (the host path decompresses, with its messages) for input the device
// does not accept or that does not fit its budget; a device failure throws.
inline std::function<bool(const std::string &, std::string &)> xz_inflater(int device, std::function<bool(const std::string &, std::string &)> other = nullptr) {
    auto ctx = std::make_shared<detail::Ctx>(device);
    return [ctx, other](const std::string &raw, std::string &out) -> bool {
        if (!detail::is_xz(raw)) return other ? other(raw, out) : false;
        return detail::stream_inflate_with(*ctx, lrge_hip_xz_inflate, {LRGE_ERR_PARSE, LRGE_ERR_TOO_MANY}, raw, out);
    };
}

inline std::vector<std::string> paf_lines(lrge_hip_ctx *ctx, const lrge_hip_index *ix, const lrge_hip_seqset *qs, int dual,
                                          const std::vector<const std::string *> &qn, const std::vector<uint32_t> &qlen,
                                          const std::vector<const std::string *> &tn, const std::vector<uint32_t> &tlen);

// overlaps.paf through a sink of text (lrge_hip_paf_text): the device formats the lines and hands them over in
// pieces of whole lines; when it cannot prove them (LRGE_ERR_UNPROVEN: a dv at a rounding boundary, an identifier above
// PAF_NAME_MAX_BYTES) the host lines of paf_lines go through the same sink instead, and nothing of the device's had been delivered.
// `hint`: room for that many chain records (0: the library's default).  `note` (may be empty) hears which path ran.  A sink that
// returns false ends the call with the reference's PafWriteError.
using PafTextSink = std::function<bool(const char *, size_t)>;
inline void paf_text(lrge_hip_ctx *ctx, const lrge_hip_index *ix, const lrge_hip_seqset *qs, int dual, const std::vector<const std::string *> &qn,
                     const std::vector<uint32_t> &qlen, const std::vector<const std::string *> &tn, const std::vector<uint32_t> &tlen, uint64_t hint,
                     const PafTextSink &sink, const std::function<void(bool)> &note) {
    auto table = [](const std::vector<const std::string *> &names, std::string &blob, std::vector<uint64_t> &off) {
        off.assign(names.size() + 1, 0);
        for (size_t i = 0; i < names.size(); ++i) off[i + 1] = off[i] + names[i]->size();
        blob.reserve(off.back());
        for (const std::string *n : names) blob += *n;
    };
    std::string qb, tb; std::vector<uint64_t> qo, to;
    table(qn, qb, qo);
    const bool same = &tn == &qn;
    if (!same) table(tn, tb, to);
    struct Fwd { const PafTextSink *sink; } fwd{&sink};
    auto cb = [](void *user, const void *bytes, uint64_t n) -> int { return (*static_cast<Fwd *>(user)->sink)(static_cast<const char *>(bytes), (size_t)n) ? 0 : 1; };
    const int rc = lrge_hip_paf_text(ctx, ix, qs, dual, qb.data(), qo.data(), same ? qb.data() : tb.data(), same ? qo.data() : to.data(), hint, cb, &fwd);
    if (rc == LRGE_ERR_UNPROVEN) {
        if (note) note(false);
        std::string piece;
        for (const std::string &l : paf_lines(ctx, ix, qs, dual, qn, qlen, tn, tlen)) {
            piece += l; piece += '\n';
            if (piece.size() >= (1u << 20)) { if (!sink(piece.data(), piece.size())) throw LrgeError(LRGE_ERR_PAF_WRITE, "Error writing PAF file: the sink refused the lines"); piece.clear(); }
        }
        if (!piece.empty() && !sink(piece.data(), piece.size())) throw LrgeError(LRGE_ERR_PAF_WRITE, "Error writing PAF file: the sink refused the lines");
        return;
    }
    if (rc) throw LrgeError(rc, lrge_hip_last_error(ctx));
    if (note) note(true);
}
// what the strategies pass as `hint`: the counts they already have, and a margin (a chain per counted overlap, some pairs chain twice)
inline uint64_t paf_chain_hint(const std::vector<uint32_t> &counts) {
    uint64_t s = 0;
    for (uint32_t c : counts) s += c;
    return s + s / 4 + 1024;
}

// ------------------------------------------------------------------------------------------
// two-set strategy
// ------------------------------------------------------------------------------------------
namespace twoset {
constexpr size_t DEFAULT_TARGET_NUM_READS = 10000, DEFAULT_QUERY_NUM_READS = 5000;   // twoset.rs:65-66

class TwoSetStrategy : public Estimate {
public:
    const Reads *input = nullptr;
    const DeviceReads *dev_input = nullptr;   // set instead of `input`: the strategy runs in the reads' own context (`device` is not used)
    size_t target_num_reads = DEFAULT_TARGET_NUM_READS, query_num_reads = DEFAULT_QUERY_NUM_READS;
    size_t target_num_bases = 0, query_num_bases = 0;
    bool remove_internal = false, use_min_ref = false;
    float max_overhang_ratio = 0.2f;
    size_t threads = 1;
    std::optional<uint64_t> seed;
    Platform platform = Platform::Nanopore;
    int device = 0;
    std::vector<std::string> warnings;
    std::vector<std::string> *paf_sink = nullptr;   // when set, receives the lines of overlaps.paf (the reference always writes it)
    PafTextSink paf_text_sink;                      // when set, overlaps.paf arrives as text formatted on the device (paf_text above); paf_sink is not filled
    std::function<void(bool)> paf_text_note;        // hears whether the device (true) or the host formatted it
    bool device_name_ranks = false;                 // name ranks by lrge_hip_name_ranks (opt-in; the host sort when the device hands them back)
    std::function<void(bool)> name_ranks_note;      // hears whether the device (true) or the host computed them, when device_name_ranks is set

    explicit TwoSetStrategy(const Reads &r) : input(&r) {}
    explicit TwoSetStrategy(const DeviceReads &r) : dev_input(&r) {}
    SampledSource *sampled = nullptr;         // set instead of either: split_fastq counts, draws and opens only the drawn reads, which become dev_input
    std::shared_ptr<DeviceReads> sampled_reads;
    explicit TwoSetStrategy(SampledSource &s) : sampled(&s) {}
    const std::vector<std::string> &names_in() const { return dev_input ? dev_input->names : input->names; }
    size_t len_in(size_t i) const { return dev_input ? dev_input->lens[i] : input->seqs[i].size(); }

    // twoset.rs:122-201
    std::tuple<std::vector<size_t>, std::vector<size_t>, float> split_fastq() {
        if (sampled && !sampled->census()) throw LrgeError(LRGE_ERR_UNPROVEN, std::string("sampled ingest: ") + lrge_hip_last_error(sampled->ctx->h));
        const size_t n = sampled ? (size_t)sampled->counts[0] : names_in().size();
        if (n > 0xFFFFFFFFull) throw LrgeError(LRGE_ERR_TOO_MANY, "Number of reads in input file exceeds maximum allowed value");
        size_t n_req = target_num_reads + query_num_reads;
        if (n <= query_num_reads)
            throw LrgeError(LRGE_ERR_TOO_FEW, "Number of reads in input file (" + std::to_string(n) + ") is <= query number of reads (" +
                                                  std::to_string(query_num_reads) + ")");
        if (n < n_req) {
            warnings.push_back("Number of reads in input file (" + std::to_string(n) + ") is less than the sum of target and query reads (" +
                               std::to_string(n_req) + ")");
            target_num_reads = n - query_num_reads;
            n_req = n;
            warnings.push_back("Using " + std::to_string(target_num_reads) + " target reads");
        }
        auto idx = detail::unique_random_set(n_req, (uint32_t)n, seed);
        // split_into_hashsets (twoset.rs:632-652): the LAST target_num_reads sampled indices are the targets
        std::unordered_set<uint32_t> tset(idx.end() - (std::ptrdiff_t)target_num_reads, idx.end()),
            qset(idx.begin(), idx.end() - (std::ptrdiff_t)target_num_reads);
        std::vector<size_t> t, q;
        if (sampled) {                     // only the drawn reads are opened: read j of the handle is record asc[j], and the lists are renumbered into 0..k-1
            std::vector<uint32_t> asc;
            sampled_reads = sampled->open(idx, &asc);
            dev_input = sampled_reads.get();
            for (size_t j = 0; j < asc.size(); ++j) {   // file order, like iter_records
                if (tset.count(asc[j])) { t.push_back(j); target_num_bases += len_in(j); }
                else { q.push_back(j); query_num_bases += len_in(j); }
            }
        } else
        for (size_t i = 0; i < n; ++i) {   // file order, like iter_records
            if (tset.count((uint32_t)i)) { t.push_back(i); target_num_bases += len_in(i); }
            else if (qset.count((uint32_t)i)) { q.push_back(i); query_num_bases += len_in(i); }
        }
        const float avg_target_len = (float)target_num_bases / (float)target_num_reads;
        return {t, q, avg_target_len};
    }

    // twoset.rs:587-606 with align_reads / align_reads_inverse replaced by the device calls
    std::pair<std::vector<float>, uint32_t> generate_estimates() override {
        auto [t, q, avg_target_len] = split_fastq();
        std::vector<const std::string *> tn, ts, qn, qs;
        for (size_t i : t) { tn.push_back(&names_in()[i]); if (input) ts.push_back(&input->seqs[i]); }
        for (size_t i : q) { qn.push_back(&names_in()[i]); if (input) qs.push_back(&input->seqs[i]); }
        std::shared_ptr<detail::Ctx> ctx_own = dev_input ? dev_input->ctx : std::make_shared<detail::Ctx>(device);
        detail::Ctx &ctx = *ctx_own;
        auto ranks = detail::name_ranks_by(ctx, device_name_ranks, name_ranks_note, {qn, tn});
        detail::SeqSet Q(ctx, dev_input, q, qs, ranks[0]), T(ctx, dev_input, t, ts, ranks[1]);
        const int preset = platform == Platform::PacBio ? LRGE_PRESET_AVA_PB : LRGE_PRESET_AVA_ONT;
        lrge_hip_params p{remove_internal ? 1 : 0, max_overhang_ratio};
        std::vector<uint32_t> counts(Q.lens.size()), has(Q.lens.size());
        uint32_t no_mapping = 0;
        if (use_min_ref && target_num_bases > query_num_bases) {
            ctx.check(lrge_hip_seqset_presketch(ctx.h, T.h, preset));   // streamed set: sketched beside the index build
            detail::Index ix(ctx, Q, preset);
            ctx.check(lrge_hip_overlap_inverse(ctx.h, ix.h, T.h, &p, counts.data()));
            if (paf_text_sink) paf_text(ctx.h, ix.h, T.h, 1, tn, T.lens, qn, Q.lens, paf_chain_hint(counts), paf_text_sink, paf_text_note);
            else if (paf_sink) *paf_sink = paf_lines(ctx.h, ix.h, T.h, 1, tn, T.lens, qn, Q.lens);
            for (uint32_t c : counts) no_mapping += c == 0;                       // twoset.rs:545-569
        } else {
            ctx.check(lrge_hip_seqset_presketch(ctx.h, Q.h, preset));
            detail::Index ix(ctx, T, preset);
            ctx.check(lrge_hip_overlap_twoset(ctx.h, ix.h, Q.h, &p, counts.data(), has.data()));
            if (paf_text_sink) paf_text(ctx.h, ix.h, Q.h, 1, qn, Q.lens, tn, T.lens, paf_chain_hint(counts), paf_text_sink, paf_text_note);
            else if (paf_sink) *paf_sink = paf_lines(ctx.h, ix.h, Q.h, 1, qn, Q.lens, tn, T.lens);
            for (uint32_t h : has) no_mapping += h == 0;                          // twoset.rs:303-309
        }
        std::vector<float> est(counts.size());
        ctx.check(lrge_hip_estimates(ctx.h, counts.data(), Q.lens.data(), (uint32_t)counts.size(), avg_target_len,
                                     target_num_reads, 100, est.data()));
        return {est, no_mapping};
    }
};

class Builder {   // twoset/builder.rs:22-185
    size_t t_ = DEFAULT_TARGET_NUM_READS, q_ = DEFAULT_QUERY_NUM_READS, threads_ = 1;
    bool remove_internal_ = false, use_min_ref_ = false;
    float ratio_ = 0.2f;
    std::optional<uint64_t> seed_;
    Platform platform_ = Platform::Nanopore;
    int device_ = 0;
    bool device_name_ranks_ = false;
    PafTextSink paf_text_sink_;
public:
    Builder &device_name_ranks(bool f) { device_name_ranks_ = f; return *this; }
    Builder &paf_text_sink(PafTextSink f) { paf_text_sink_ = std::move(f); return *this; }
    Builder &target_num_reads(size_t n) { t_ = n; return *this; }
    Builder &query_num_reads(size_t n) { q_ = n; return *this; }
    Builder &remove_internal(bool f, float ratio) { remove_internal_ = f; if (f) ratio_ = ratio; return *this; }
    Builder &use_min_ref(bool f) { use_min_ref_ = f; return *this; }
    Builder &threads(size_t n) { threads_ = n; return *this; }
    Builder &seed(std::optional<uint64_t> s) { seed_ = s; return *this; }
    Builder &platform(Platform p) { platform_ = p; return *this; }
    Builder &device(int d) { device_ = d; return *this; }
    TwoSetStrategy build(const Reads &input) const { return configure(TwoSetStrategy(input)); }
    TwoSetStrategy build(const DeviceReads &input) const { return configure(TwoSetStrategy(input)); }
    TwoSetStrategy build(SampledSource &input) const { return configure(TwoSetStrategy(input)); }
    TwoSetStrategy configure(TwoSetStrategy s) const {
        s.target_num_reads = t_; s.query_num_reads = q_; s.remove_internal = remove_internal_; s.max_overhang_ratio = ratio_;
        s.use_min_ref = use_min_ref_; s.threads = threads_; s.seed = seed_; s.platform = platform_; s.device = device_;
        s.device_name_ranks = device_name_ranks_;
        s.paf_text_sink = paf_text_sink_;
        return s;
    }
};
}  // namespace twoset

// ------------------------------------------------------------------------------------------
// all-vs-all strategy
// ------------------------------------------------------------------------------------------
namespace ava {
constexpr size_t DEFAULT_AVA_NUM_READS = 25000;   // ava.rs:62

class AvaStrategy : public Estimate {
public:
    const Reads *input = nullptr;
    const DeviceReads *dev_input = nullptr;   // as TwoSetStrategy::dev_input
    size_t num_reads = DEFAULT_AVA_NUM_READS, num_bases = 0, threads = 1;
    bool remove_internal = false;
    float max_overhang_ratio = 0.2f;
    std::optional<uint64_t> seed;
    Platform platform = Platform::Nanopore;
    int device = 0;
    std::vector<std::string> warnings;
    std::vector<std::string> *paf_sink = nullptr;
    PafTextSink paf_text_sink;                      // as TwoSetStrategy::paf_text_sink
    std::function<void(bool)> paf_text_note;
    bool device_name_ranks = false;                 // as TwoSetStrategy::device_name_ranks
    std::function<void(bool)> name_ranks_note;

    explicit AvaStrategy(const Reads &r) : input(&r) {}
    explicit AvaStrategy(const DeviceReads &r) : dev_input(&r) {}
    SampledSource *sampled = nullptr;         // as TwoSetStrategy::sampled
    std::shared_ptr<DeviceReads> sampled_reads;
    explicit AvaStrategy(SampledSource &s) : sampled(&s) {}

    std::pair<std::vector<float>, uint32_t> generate_estimates() override {
        // ava.rs:108-161
        if (sampled && !sampled->census()) throw LrgeError(LRGE_ERR_UNPROVEN, std::string("sampled ingest: ") + lrge_hip_last_error(sampled->ctx->h));
        const size_t n = sampled ? (size_t)sampled->counts[0] : (dev_input ? dev_input->names : input->names).size();
        if (n > 0xFFFFFFFFull) throw LrgeError(LRGE_ERR_TOO_MANY, "Number of reads in input file exceeds maximum allowed value");
        if (n < num_reads) {
            warnings.push_back("Number of reads in input file (" + std::to_string(n) + ") is less than the number requested (" +
                               std::to_string(num_reads) + ")");
            num_reads = n;
        }
        auto idx = detail::unique_random_set(num_reads, (uint32_t)n, seed);
        std::unordered_set<uint32_t> keep(idx.begin(), idx.end());
        std::vector<const std::string *> rn, rs;
        std::vector<size_t> ri;
        if (sampled) {                     // only the drawn reads are opened, in file order: all of the handle's reads are the sample
            std::vector<uint32_t> asc;
            sampled_reads = sampled->open(idx, &asc);
            dev_input = sampled_reads.get();
            for (size_t j = 0; j < asc.size(); ++j) { rn.push_back(&dev_input->names[j]); ri.push_back(j); num_bases += dev_input->lens[j]; }
        }
        const std::vector<std::string> &names = sampled ? dev_input->names : dev_input ? dev_input->names : input->names;
        if (!sampled)
        for (size_t i = 0; i < n; ++i) if (keep.count((uint32_t)i)) {
            rn.push_back(&names[i]); ri.push_back(i);
            if (input) rs.push_back(&input->seqs[i]);
            num_bases += dev_input ? dev_input->lens[i] : input->seqs[i].size();
        }
        // ava.rs:369-382 + :165-366
        std::shared_ptr<detail::Ctx> ctx_own = dev_input ? dev_input->ctx : std::make_shared<detail::Ctx>(device);
        detail::Ctx &ctx = *ctx_own;
        auto ranks = detail::name_ranks_by(ctx, device_name_ranks, name_ranks_note, {rn});
        detail::SeqSet R(ctx, dev_input, ri, rs, ranks[0]);
        const int preset = platform == Platform::PacBio ? LRGE_PRESET_AVA_PB : LRGE_PRESET_AVA_ONT;
        ctx.check(lrge_hip_seqset_presketch(ctx.h, R.h, preset));
        detail::Index ix(ctx, R, preset);
        lrge_hip_params p{remove_internal ? 1 : 0, max_overhang_ratio};
        std::vector<uint32_t> counts(R.lens.size());
        ctx.check(lrge_hip_overlap_ava(ctx.h, ix.h, R.h, &p, counts.data()));
        if (paf_text_sink) paf_text(ctx.h, ix.h, R.h, 0, rn, R.lens, rn, R.lens, paf_chain_hint(counts), paf_text_sink, paf_text_note);
        else if (paf_sink) *paf_sink = paf_lines(ctx.h, ix.h, R.h, 0, rn, R.lens, rn, R.lens);
        const size_t n_target = num_reads - 1;                                   // ava.rs:339-346
        const float avg = (float)num_bases / (float)n_target;
        std::vector<float> est(counts.size());
        ctx.check(lrge_hip_estimates(ctx.h, counts.data(), R.lens.data(), (uint32_t)counts.size(), avg, n_target, 100, est.data()));
        uint32_t no_mapping = 0;
        for (uint32_t c : counts) no_mapping += c == 0;                          // ava.rs:329-331
        return {est, no_mapping};
    }
};

class Builder {   // ava/builder.rs:19-153
    size_t n_ = DEFAULT_AVA_NUM_READS, threads_ = 1;
    bool remove_internal_ = false;
    float ratio_ = 0.2f;
    std::optional<uint64_t> seed_;
    Platform platform_ = Platform::Nanopore;
    int device_ = 0;
    bool device_name_ranks_ = false;
    PafTextSink paf_text_sink_;
public:
    Builder &device_name_ranks(bool f) { device_name_ranks_ = f; return *this; }
    Builder &paf_text_sink(PafTextSink f) { paf_text_sink_ = std::move(f); return *this; }
    Builder &num_reads(size_t n) { n_ = n; return *this; }
    Builder &remove_internal(bool f, float ratio) { remove_internal_ = f; if (f) ratio_ = ratio; return *this; }
    Builder &threads(size_t n) { threads_ = n; return *this; }
    Builder &seed(std::optional<uint64_t> s) { seed_ = s; return *this; }
    Builder &platform(Platform p) { platform_ = p; return *this; }
    Builder &device(int d) { device_ = d; return *this; }
    AvaStrategy build(const Reads &input) const { return configure(AvaStrategy(input)); }
    AvaStrategy build(const DeviceReads &input) const { return configure(AvaStrategy(input)); }
    AvaStrategy build(SampledSource &input) const { return configure(AvaStrategy(input)); }
    AvaStrategy configure(AvaStrategy s) const {
        s.num_reads = n_; s.remove_internal = remove_internal_; s.max_overhang_ratio = ratio_; s.threads = threads_;
        s.seed = seed_; s.platform = platform_; s.device = device_;
        s.device_name_ranks = device_name_ranks_;
        s.paf_text_sink = paf_text_sink_;
        return s;
    }
};
}  // namespace ava

// the lines of overlaps.paf from n chain records and the per-query statistics (mapping.rs:81-177), no line feed
inline std::vector<std::string> paf_format_lines(const lrge_hip_chain *ch, uint64_t n, const int32_t *rl, const uint64_t *ss, const uint32_t *nk,
                                                 const std::vector<const std::string *> &qn, const std::vector<uint32_t> &qlen,
                                                 const std::vector<const std::string *> &tn, const std::vector<uint32_t> &tlen) {
    std::vector<std::string> out;
    char buf[512];
    for (uint64_t i = 0; i < n; ++i) {
        const lrge_hip_chain &c = ch[i];
        const uint32_t q = c.query, t = c.target;
        float dv = -1.0f;                                     // mm2:esterr.c mm_est_err
        if (nk[q]) {
            const float avg_k = (float)ss[q] / (float)nk[q];
            int n_tot = c.n_seeds;
            if ((float)c.qs > avg_k && (float)c.rs > avg_k) ++n_tot;
            if ((float)((int)qlen[q] - c.qs) > avg_k && (float)((int)tlen[t] - c.re) > avg_k) ++n_tot;
            dv = c.cnt >= n_tot ? 0.0f : (float)(1.0 - std::pow((double)c.cnt / n_tot, 1.0 / avg_k));
        }
        char dvs[32];
        if (dv < 1.1920929e-07f) snprintf(dvs, sizeof(dvs), "0"); else snprintf(dvs, sizeof(dvs), "%.4f", (double)dv);   // mapping.rs:136-147
        snprintf(buf, sizeof(buf), "\t%u\t%d\t%d\t%c\t", qlen[q], c.qs, c.qe, c.rev ? '-' : '+');
        std::string line = *qn[q] + buf + *tn[t];
        snprintf(buf, sizeof(buf), "\t%u\t%d\t%d\t%d\t%d\t0\ttp:A:S\tcm:i:%d\ts1:i:%d\tdv:f:%s\trl:i:%d", tlen[t], c.rs, c.re, c.mlen, c.blen,
                 c.cnt, c.score, dvs, rl[q]);
        out.push_back(line + buf);
    }
    return out;
}

// overlaps.paf (twoset.rs:246-250,289-293; mapping.rs:81-177): one line per chain, unordered like the reference
inline std::vector<std::string> paf_lines(lrge_hip_ctx *ctx, const lrge_hip_index *ix, const lrge_hip_seqset *qs, int dual,
                                          const std::vector<const std::string *> &qn, const std::vector<uint32_t> &qlen,
                                          const std::vector<const std::string *> &tn, const std::vector<uint32_t> &tlen) {
    uint64_t n = 0;
    int rc = lrge_hip_chains(ctx, ix, qs, dual, nullptr, 0, &n);
    if (rc) throw LrgeError(rc, lrge_hip_last_error(ctx));
    std::vector<lrge_hip_chain> ch(n ? n : 1);
    rc = lrge_hip_chains(ctx, ix, qs, dual, ch.data(), n, &n);
    if (rc) throw LrgeError(rc, lrge_hip_last_error(ctx));
    std::vector<int32_t> rl(qn.size() + 1); std::vector<uint64_t> ss(qn.size() + 1); std::vector<uint32_t> nk(qn.size() + 1);
    rc = lrge_hip_paf_stats(ctx, ix, qs, rl.data(), ss.data(), nk.data());
    if (rc) throw LrgeError(rc, lrge_hip_last_error(ctx));
    return paf_format_lines(ch.data(), n, rl.data(), ss.data(), nk.data(), qn, qlen, tn, tlen);
}

// lrge/src/utils.rs:19-49
inline std::string format_estimate(float estimate) {
    if (std::isinf(estimate)) return "\xE2\x88\x9E bp";
    static const char *units[] = {"bp", "kbp", "Mbp", "Gbp", "Tbp", "Pbp"};
    float value = estimate; const char *suffix = "bp";
    for (int power = 0; power < 6; ++power) {
        const float threshold = std::pow(10.0f, (float)(power * 3));
        if (estimate >= threshold) { value = estimate / threshold; suffix = units[power]; } else break;
    }
    char buf[64];
    snprintf(buf, sizeof(buf), "%.2f %s", value, suffix);
    return buf;
}

}  // namespace lrge
