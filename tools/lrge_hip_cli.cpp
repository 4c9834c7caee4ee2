// lrge_hip_cli.cpp -- flag-for-flag mirror of the `lrge` command line (lrge/src/cli.rs:9-87,
// lrge/src/main.rs:32-123) driving the MI355X overlap engine through include/lrge_hip.hpp.
// Input: FASTA / FASTQ / unaligned SAM / unaligned BAM, plain or gzip / bzip2 / xz / zstd compressed, sniffed by
// magic bytes like liblrge/src/io.rs (include/lrge_io.hpp; CRAM is recognised and refused).  Like the reference CLI, -P is parsed but NOT forwarded to the
// builders (lrge/src/main.rs:56-85), so the preset is always ava-ont; pass --honour-platform to
// forward it (what the library API does).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <cmath>
#include <iostream>

#include "../include/lrge_hip.hpp"
#include "../include/lrge_io.hpp"

static lrge::Reads load_reads(const std::string &path, bool gpu_inflate, bool gpu_gzip, bool gpu_bzip2, bool gpu_zstd, bool gpu_xz, int device) {   // io.rs:154-184 via include/lrge_io.hpp
    lrge::Reads r;
    try {
        auto add = [&](const std::string &name, const std::string &seq) { r.names.push_back(name); r.seqs.push_back(seq); };
        // gzip as its two flags say (every gzip input, or BGZF alone), then bzip2, Zstandard and xz in front of it, each on the device by its own flag
        std::function<bool(const std::string &, std::string &)> hook = gpu_gzip ? lrge::gzip_inflater(device) : gpu_inflate ? lrge::bgzf_inflater(device) : nullptr;
        if (gpu_bzip2) hook = lrge::bzip2_inflater(device, hook);
        if (gpu_zstd) hook = lrge::zstd_inflater(device, hook);
        if (gpu_xz) hook = lrge::xz_inflater(device, hook);
        if (hook) lrge::io::iter_records(path, add, hook);
        else lrge::io::iter_records(path, add);
    } catch (const lrge::io::IoError &e) {
        throw lrge::LrgeError(LRGE_ERR_IO, e.what());
    }
    if (r.names.empty()) throw lrge::LrgeError(LRGE_ERR_IO, "IO error: Is the file empty?");   // count_records, io.rs:140-145
    return r;
}

// Rust's `{}` for an f32 (main.rs:107): the shortest decimal digits that read back as the same f32, written positionally
// (never with an exponent).
static std::string display_f32(float v) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
    char buf[64];
    int prec = 0;
    for (; prec < 9; ++prec) {
        snprintf(buf, sizeof buf, "%.*e", prec, (double)v);
        if (strtof(buf, nullptr) == v) break;
    }
    snprintf(buf, sizeof buf, "%.*e", prec, (double)v);
    std::string m(buf);
    const size_t epos = m.find('e');
    const int ex = atoi(m.c_str() + epos + 1);
    std::string digits; bool neg = false;
    for (size_t i = 0; i < epos; ++i) { if (m[i] == '-') neg = true; else if (m[i] != '.') digits += m[i]; }
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();      // 1.50e3 -> "15", exponent 3
    std::string out;
    if (ex >= 0) {
        if ((int)digits.size() <= ex + 1) out = digits + std::string((size_t)(ex + 1 - (int)digits.size()), '0');
        else out = digits.substr(0, (size_t)ex + 1) + "." + digits.substr((size_t)ex + 1);
    } else out = "0." + std::string((size_t)(-ex - 1), '0') + digits;
    return (neg ? "-" : "") + out;
}

int main(int argc, char **argv) {
    std::string input, output = "-", platform = "ont";
    std::optional<size_t> T = 10000, Q = 5000, N;
    bool T_set = false, Q_set = false, filter = false, with_inf = false, precise = false, use_min_ref = false, honour_platform = false;
    float q1 = lrge::LOWER_QUANTILE, q3 = lrge::UPPER_QUANTILE, ratio = 0.2f;
    size_t threads = 1; std::optional<uint64_t> seed; int quiet = 0, verbose = 0, device = 0;
    bool keep_temp = false, dump_records = false, gpu_inflate = false, gpu_gzip = false, gpu_bzip2 = false, gpu_zstd = false, gpu_xz = false, gpu_cram = false, gpu_ingest = false, gpu_sample = false, gpu_seek = false, gpu_stream = false, gpu_names = false, gpu_paf = false; std::string temp_dir;
    auto need = [&](int &i) -> const char * { if (i + 1 >= argc) { fprintf(stderr, "error: missing value for %s\n", argv[i]); exit(2); } return argv[++i]; };
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "-o" || a == "--output") output = need(i);
        else if (a == "-T" || a == "--target") { T = strtoull(need(i), 0, 10); T_set = true; }
        else if (a == "-Q" || a == "--query") { Q = strtoull(need(i), 0, 10); Q_set = true; }
        else if (a == "-n" || a == "--num") N = strtoull(need(i), 0, 10);
        else if (a == "-P" || a == "--platform") { platform = need(i); if (platform != "ont" && platform != "pb") { fprintf(stderr, "error: invalid platform\n"); return 2; } }
        else if (a == "-F" || a == "--filter-contained") filter = true;
        else if (a == "-t" || a == "--threads") threads = strtoull(need(i), 0, 10);
        else if (a == "-C" || a == "--keep-temp") keep_temp = true;
        else if (a == "-D" || a == "--temp") temp_dir = need(i);
        else if (a == "-s" || a == "--seed") seed = strtoull(need(i), 0, 10);
        else if (a == "-8" || a == "--inf") with_inf = true;
        else if (a == "-f" || a == "--float-my-boat") precise = true;
        else if (a == "--q1") q1 = strtof(need(i), 0);
        else if (a == "--q3") q3 = strtof(need(i), 0);
        else if (a == "--max-overhang-ratio") ratio = strtof(need(i), 0);
        else if (a == "--use-min-ref") use_min_ref = true;
        else if (a == "--honour-platform") honour_platform = true;
        else if (a == "--device") device = atoi(need(i));
        else if (a == "--gpu-inflate") gpu_inflate = true;       // BGZF input (BAM, bgzip FASTQ) decompressed on --device
        else if (a == "--gpu-gzip") gpu_gzip = true;             // every gzip input (plain, multi-member, BGZF) decompressed on --device
        else if (a == "--gpu-xz") gpu_xz = true;                 // xz input decompressed on --device (with --gpu-ingest: kept in HBM); not implied by --gpu-ingest
        else if (a == "--gpu-cram") gpu_cram = true;             // beside --gpu-ingest: unaligned CRAM walked on the host, its base blocks decoded on --device; not implied by --gpu-ingest
        else if (a == "--gpu-zstd") gpu_zstd = true;             // Zstandard input decompressed on --device (with --gpu-ingest: kept in HBM, through the windows and -- with --gpu-sample -- the sampled route: LRGE_GPU_INGEST_WINDOWED_ZSTD); not implied by --gpu-ingest
        else if (a == "--gpu-bzip2") gpu_bzip2 = true;           // bzip2 input decompressed on --device (with --gpu-ingest: kept in HBM)
        else if (a == "--gpu-ingest") { gpu_ingest = true; gpu_gzip = true; }   // FASTA / FASTQ / unaligned BAM / unaligned SAM parsed on --device too: the bases never reach host memory (implies --gpu-gzip)
        else if (a == "--gpu-sample") gpu_sample = true;         // beside --gpu-ingest: a count pass, then only the drawn reads are kept (lrge_hip_reads_census, lrge_hip_reads_open_selected); not implied by --gpu-ingest
        else if (a == "--gpu-seek") gpu_seek = true;             // beside --gpu-sample: the count pass keeps a seek map, the second pass reads and decodes only the runs of plain / BGZF input, the entries of gzip and (with --gpu-bzip2) the blocks of bzip2 that hold drawn reads (lrge_hip_reads_census_map, lrge_hip_reads_open_mapped)
        else if (a == "--gpu-stream") gpu_stream = true;         // beside --gpu-ingest: the first pass reads plain, BGZF and gzip input in pinned pieces instead of whole (LRGE_GPU_INGEST_STREAM, option INGEST_STREAM_BYTES); not implied by --gpu-ingest
        else if (a == "--gpu-names") gpu_names = true;           // identifier ranks computed on --device (lrge_hip_name_ranks); not implied by --gpu-ingest
        else if (a == "--gpu-paf") gpu_paf = true;               // beside -C: overlaps.paf is formatted on --device and written piece by piece (lrge_hip_paf_text); without -C it has no effect; not implied by --gpu-ingest
        else if (a == "--dump-records") dump_records = true;   // host-only: print "id<TAB>sequence" per record and exit (tests)
        else if (a == "-q" || a == "--quiet") ++quiet; else if (a == "-qq") quiet += 2; else if (a == "-qqq") quiet += 3;
        else if (a == "-v" || a == "--verbose") ++verbose; else if (a == "-vv") verbose += 2;
        else if (!a.empty() && a[0] == '-' && a != "-") { fprintf(stderr, "error: unexpected argument '%s'\n", a.c_str()); return 2; }
        else input = a;
    }
    if (input.empty()) { fprintf(stderr, "error: the following required arguments were not provided: <INPUT>\n"); return 2; }
    if (N && (T_set || Q_set)) { fprintf(stderr, "error: the argument '--num <INT>' cannot be used with '--target'/'--query'\n"); return 2; }
    if (!(q1 >= 0.f && q1 <= 0.5f) || !(q3 >= 0.5f && q3 <= 1.f) || !(ratio >= 0.f && ratio <= 1.f)) { fprintf(stderr, "error: quantile/ratio out of range\n"); return 2; }
    if (gpu_sample && !gpu_ingest) { fprintf(stderr, "error: the argument '--gpu-sample' requires '--gpu-ingest'\n"); return 2; }
    if (gpu_seek && !gpu_sample) { fprintf(stderr, "error: the argument '--gpu-seek' requires '--gpu-sample'\n"); return 2; }
    if (gpu_stream && !gpu_ingest) { fprintf(stderr, "error: the argument '--gpu-stream' requires '--gpu-ingest'\n"); return 2; }
    if (quiet && verbose) { fprintf(stderr, "error: --quiet cannot be used with --verbose\n"); return 2; }
    const bool info = quiet == 0;
    try {
        if (dump_records) {
            size_t n = lrge::io::count_records(input);
            lrge::io::iter_records(input, [](const std::string &name, const std::string &seq) { printf("%s\t%s\n", name.c_str(), seq.c_str()); });
            fprintf(stderr, "%zu records\n", n);
            return 0;
        }
        // --gpu-ingest: input the device does not prove takes the usual route below, which parses it or reports it
        std::unique_ptr<lrge::DeviceReads> dev;
        // --gpu-sample beside it: the census counts the records, the strategy opens only the reads it draws; input the two passes
        // do not prove takes the route of --gpu-ingest alone
        std::unique_ptr<lrge::SampledSource> sampled;
        if (gpu_ingest) {
            const int fl = LRGE_GPU_INFLATE_BGZF | LRGE_GPU_INFLATE_GZIP | LRGE_GPU_INGEST_BAM | LRGE_GPU_INGEST_SAM | LRGE_GPU_INGEST_WINDOWED | LRGE_GPU_INGEST_WINDOWED_ALN | (gpu_bzip2 ? LRGE_GPU_INFLATE_BZIP2 : 0) | (gpu_zstd ? LRGE_GPU_INFLATE_ZSTD | LRGE_GPU_INGEST_WINDOWED_ZSTD : 0) | (gpu_xz ? LRGE_GPU_INFLATE_XZ : 0) | (gpu_cram ? LRGE_GPU_INGEST_CRAM : 0) | (gpu_stream ? LRGE_GPU_INGEST_STREAM : 0);
            if (gpu_sample) {
                sampled.reset(new lrge::SampledSource{input, fl | LRGE_GPU_INGEST_SELECT_ALN | LRGE_GPU_INGEST_SELECT_SAM | (gpu_cram ? LRGE_GPU_INGEST_SELECT_CRAM : 0), device});       // (unaligned BAM, SAM and -- with --gpu-cram -- CRAM take the sampled route too: DESIGN sections 25 and 27)
                sampled->seek = gpu_seek;
                if (!sampled->census()) sampled.reset();
                else if (!sampled->counts[0]) throw lrge::LrgeError(LRGE_ERR_IO, "IO error: Is the file empty?");
            }
            if (!sampled) dev = lrge::DeviceReads::open(input, fl, device);
            if (info) fprintf(stderr, "[INFO] gpu-ingest: %s\n", sampled ? (gpu_seek ? "device (sampled, seek)" : "device (sampled)") : dev ? "device" : "host");
            if (dev && dev->names.empty()) throw lrge::LrgeError(LRGE_ERR_IO, "IO error: Is the file empty?");
        }
        lrge::Reads reads;
        if (!dev && !sampled) reads = load_reads(input, gpu_inflate, gpu_gzip, gpu_bzip2, gpu_zstd, gpu_xz, device);
        const lrge::Platform pf = (honour_platform && platform == "pb") ? lrge::Platform::PacBio : lrge::Platform::Nanopore;
        lrge::twoset::TwoSetStrategy ts = dev ? lrge::twoset::TwoSetStrategy(*dev) : lrge::twoset::TwoSetStrategy(reads);
        lrge::ava::AvaStrategy as = dev ? lrge::ava::AvaStrategy(*dev) : lrge::ava::AvaStrategy(reads);
        lrge::Estimate *st;
        const std::function<void(bool)> names_note = [&](bool on_device) { if (info) fprintf(stderr, "[INFO] gpu-names: %s\n", on_device ? "device" : "host"); };
        if (N) {
            if (info) fprintf(stderr, "[INFO] Running all-vs-all strategy with %zu reads\n", *N);
            const auto b = lrge::ava::Builder().num_reads(*N).remove_internal(filter, ratio).threads(threads).seed(seed).platform(pf).device(device).device_name_ranks(gpu_names);
            as = sampled ? b.build(*sampled) : dev ? b.build(*dev) : b.build(reads);
            as.name_ranks_note = names_note;
            st = &as;
        } else {
            if (info) fprintf(stderr, "[INFO] Running two-set strategy with %zu target reads and %zu query reads\n", *T, *Q);
            const auto b = lrge::twoset::Builder().target_num_reads(*T).query_num_reads(*Q).remove_internal(filter, ratio).use_min_ref(use_min_ref)
                               .threads(threads).seed(seed).platform(pf).device(device).device_name_ranks(gpu_names);
            ts = sampled ? b.build(*sampled) : dev ? b.build(*dev) : b.build(reads);
            ts.name_ranks_note = names_note;
            st = &ts;
        }
        std::vector<std::string> paf;
        const std::string dir = temp_dir.empty() ? "." : temp_dir;
        std::ofstream paf_out;
        if (keep_temp && gpu_paf) {      // the pieces go straight to the file as the device hands them over
            paf_out.open(dir + "/overlaps.paf", std::ios::binary);
            if (!paf_out) { fprintf(stderr, "Error: Failed to write PAF record\n"); return 1; }
            const lrge::PafTextSink to_file = [&](const char *p, size_t n) { paf_out.write(p, (std::streamsize)n); return (bool)paf_out; };
            const std::function<void(bool)> paf_note = [&](bool on_device) { if (info) fprintf(stderr, "[INFO] gpu-paf: %s\n", on_device ? "device" : "host"); };
            ts.paf_text_sink = to_file; as.paf_text_sink = to_file; ts.paf_text_note = paf_note; as.paf_text_note = paf_note;
        } else if (keep_temp) { ts.paf_sink = &paf; as.paf_sink = &paf; }   // -C keeps overlaps.paf (main.rs:37-48, twoset.rs:246-250)
        lrge::EstimateResult r = st->estimate(!with_inf, q1, q3);
        if (keep_temp && gpu_paf) {
            paf_out.close();
            if (!paf_out) { fprintf(stderr, "Error: Failed to generate estimate\n\nCaused by:\n    Error writing PAF file: closing %s/overlaps.paf failed\n", dir.c_str()); return 1; }
            if (info) fprintf(stderr, "[INFO] Created temporary directory at %s\n", dir.c_str());
        } else if (keep_temp) {
            std::ofstream pf(dir + "/overlaps.paf");
            if (!pf) { fprintf(stderr, "Error: Failed to write PAF record\n"); return 1; }
            for (auto &l : paf) pf << l << "\n";
            if (info) fprintf(stderr, "[INFO] Created temporary directory at %s\n", dir.c_str());
        }
        if (quiet < 2) for (auto &w : (N ? as.warnings : ts.warnings)) fprintf(stderr, "[WARN] %s\n", w.c_str());
        if (!r.estimate) { fprintf(stderr, "Error: %s\n", with_inf ? "No estimates were generated" : "No finite estimates were generated"); return 1; }
        if (info) {
            std::string msg = "Estimated genome size: " + lrge::format_estimate(*r.estimate);
            if (r.lower && r.upper) msg += " (IQR: " + lrge::format_estimate(*r.lower) + " - " + lrge::format_estimate(*r.upper) + ")";
            fprintf(stderr, "[INFO] %s\n", msg.c_str());
        }
        FILE *out = output == "-" ? stdout : fopen(output.c_str(), "w");
        if (!out) { fprintf(stderr, "Error: Failed to create output file\n"); return 1; }
        if (precise) fprintf(out, "%s\n", display_f32(*r.estimate).c_str()); else fprintf(out, "%.0f\n", (double)*r.estimate);
        if (out != stdout) fclose(out);
        if (info) fprintf(stderr, "[INFO] Done!\n");
    } catch (const lrge::io::IoError &e) {
        fprintf(stderr, "Error: Failed to generate estimate\n\nCaused by:\n    %s\n", e.what());
        return 1;
    } catch (const lrge::LrgeError &e) {
        fprintf(stderr, "Error: Failed to generate estimate\n\nCaused by:\n    %s\n", e.what());
        return 1;
    }
    return 0;
}
