// gx-align -- the reference CLI (src/main.rs) on top of the C ABI.
//
//   gx-align [-c config.toml] align [-a local|global|1] -f pair.fasta
//       main.rs:27-37, 77-84, 86-153: load config (config.rs) and FASTA
//       (sequence.rs), align the first two records on the GPU, print the
//       sequence table for small inputs (retrace -> print_alignment_table,
//       algo.rs:438, display.rs:131-220) and the AlignedSequences Display
//       (display.rs:9-127).
//
//   gx-align [-c config.toml] all-vs-all -d fasta_dir [-a global|local]
//            [-o similarity_matrix.tsv] [-g N_GPUS] [--no-self]
//       BASELINE config 4: every pair (i, j), i <= j, of the
//       records of all *.fasta files in fasta_dir aligned on the GPU(s), with
//       the matrix layout and TSV writer of the reference's `compare` mode
//       (main.rs:216-378: row r, column c filled for c <= r, written as
//       "r\t v\t v\t ..."), carrying the alignment score instead of the suffix
//       tree's LCS score.  Pairs are sharded over the GPUs by longest-
//       processing-time on n*m, one host thread and gx_context per GPU, one
//       batched launch per GPU.  Files are read in name order (the reference
//       uses fs::read_dir order, which the OS leaves unspecified).
//
//   gx-align compare -d fasta_dir [-o similarity_matrix.tsv]
//       main.rs:216-379: the similarity matrix of the records of all *.fasta
//       files in fasta_dir (name order, as all-vs-all) -- element [j][i], i <= j,
//       is the sum of longest-common-substring lengths over the reference's
//       recursion (gx_compare_matrix) -- written as similarity_matrix.tsv and
//       printed as the "Similarity TSV" and "LCS Length TSV" blocks
//       (main.rs:330-378).  The alphabet file, suffix-link and thread options
//       configure the reference's suffix tree and thread pool and have no
//       counterpart; its coloured overview (comparison/display.rs) is not
//       printed.
//
//   gx-align suffix-tree -f file.fasta [-a alphabet.txt] [--suffix-links] [--stats] [-o bwt.txt]
//       main.rs:154-215: the suffix tree of the file's first record, read off
//       its suffix array (gx_suffix_tree_stats).  With --stats the BWT is
//       written one character per line (BWT_out/<name>_bwt.txt unless -o) and
//       the "Stats:" block is printed.  An alphabet file, when given, is
//       checked as the reference's tree checks it; --suffix-links is accepted
//       and ignored; the Graphviz block of small trees is not printed.
//
//   gx-align [-c config.toml] search -f genome.fasta -p patterns.fasta [--max-hits K] [-k MISMATCHES | -e EDITS [--cigar]] [-o hits.tsv]
//       No counterpart in the reference's main.rs: where every record of
//       patterns.fasta occurs in the first record of genome.fasta, from a
//       suffix index kept on the GPU (gx_suffix_index_search).
//       One TSV line per pattern, to stdout unless -o: name, length, count,
//       prefix_len, prefix_pos and up to K (default 16) 0-based ascending
//       positions, comma-separated.  With -k: every start where the pattern
//       matches with at most that many substitutions
//       (gx_suffix_index_search_approx); the line is then name,
//       length, count, best_dist, best_pos and up to K pos:dist pairs.  With -e
//       (not together with -k): every end where the pattern matches with at
//       most that many substitutions, insertions and deletions
//       (gx_suffix_index_search_edit); the line is then name,
//       length, count, best_dist, best_end and up to K start-end:dist triples.
//       With --cigar (with -e alone) every reported window is aligned to its
//       pattern on the band of EDITS diagonals under the scores of the config
//       file (gx_suffix_index_extend) and a triple becomes
//       start-end:dist:score:CIGAR.
//   gx-align search -f genome.fasta -p queries.fasta --mem L [-o mems.tsv]
//       (not together with -k or -e) Every maximal exact match of L bases or
//       more between a record of queries.fasta, of any length, and the genome
//       (gx_suffix_index_mems).  One line per MEM: query name,
//       qpos, tpos, len (0-based), by query, then qpos, then tpos; after them
//       one line per query without a MEM: name, -, -, 0.
//   gx-align search ... --mem L --chain [--chain-gap G] [--chain-drift D] [--chain-pred H] [--chain-min-score S]
//       The MEMs of every query chained into colinear chains (gx_chain_anchors,
//       DESIGN.md 23; max_gap, max_drift, max_pred and min_score, the library's
//       defaults where not given).  One line per chain instead of the MEMs:
//       query name, chain number within the query, score, n_anchors, qstart,
//       qend, tstart, tend; after them one line per query without a chain:
//       name, -, 0.
//   gx-align search ... --strands forward|reverse|both
//       In every sub-mode above: the records are searched on the chosen strands
//       (the _strands calls).  A line per item: with "both" every
//       record on the forward strand first, then every record's reverse
//       complement.  Every line gains a strand column, + or -, directly behind
//       the name; with --mem and --chain the record's length follows it, since a
//       - line's qpos counts in the reverse complement (the same bases begin at
//       length - qpos - len in the record).  Text positions are the forward
//       genome's.  Without the flag the output is what it always was.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/gx.h"

namespace {

void usage() {
    fprintf(stderr,
            "Usage: gx-align [-c|--config-path <CONFIG>] align [-a|--alignment-type <TYPE>] -f|--fasta-path <FASTA>\n"
            "       gx-align [-c|--config-path <CONFIG>] all-vs-all -d|--fasta-dir <DIR> [-a <TYPE>] "
            "[-o <TSV>] [-g|--gpus <N>] [--no-self]\n"
            "       gx-align compare -d|--fasta-dir <DIR> [-o <TSV>]\n"
            "       gx-align suffix-tree -f|--fasta-path <FASTA> [-a|--alphabet-file <ALPHABET>] [--suffix-links] "
            "[--stats] [-o <BWT>]\n"
            "       gx-align search -f|--fasta-path <GENOME> -p|--patterns <PATTERNS> [--max-hits <K>] [-k <MISMATCHES> | -e <EDITS> [--cigar]] [--strands forward|reverse|both] [-o <TSV>]\n"
            "       gx-align search -f|--fasta-path <GENOME> -p|--patterns <QUERIES> --mem <MIN_LEN> [--chain [--chain-gap <G>] "
            "[--chain-drift <D>] [--chain-pred <H>] [--chain-min-score <S>]] [--strands forward|reverse|both] [-o <TSV>]\n");
}

struct Records {
    std::vector<uint8_t> buf;
    std::vector<uint64_t> no, nl, so, sl;
    size_t size() const { return so.size(); }
    const uint8_t* seq(size_t k) const { return buf.data() + so[k]; }
    std::string name(size_t k) const { return std::string((const char*)buf.data() + no[k], nl[k]); }
};

// from_fasta (sequence.rs:45-95) appending to `r`
void load_fasta(const std::string& path, Records& r) {
    size_t nrec = 0, need = 0;
    gx_fasta_load(path.c_str(), nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, &nrec, &need);
    if (!nrec) return;
    std::vector<uint8_t> buf(need + 1);
    std::vector<uint64_t> no(nrec), nl(nrec), so(nrec), sl(nrec);
    gx_fasta_load(path.c_str(), buf.data(), buf.size(), no.data(), nl.data(), so.data(), sl.data(), nrec, &nrec,
                  &need);
    const uint64_t base = r.buf.size();
    r.buf.insert(r.buf.end(), buf.begin(), buf.begin() + need);
    for (size_t k = 0; k < nrec; ++k) {
        r.no.push_back(base + no[k]);
        r.nl.push_back(nl[k]);
        r.so.push_back(base + so[k]);
        r.sl.push_back(sl[k]);
    }
}

bool stdout_color() {
    // the `colored` crate: CLICOLOR_FORCE forces, NO_COLOR / CLICOLOR=0 disable, else a terminal
    if (const char* f = getenv("CLICOLOR_FORCE"); f && strcmp(f, "0")) return true;
    if (const char* nc = getenv("NO_COLOR"); nc && *nc) return false;
    if (const char* c = getenv("CLICOLOR"); c && !strcmp(c, "0")) return false;
    return isatty(1);
}

int fail_msg(const char* what, int rc) {
    fprintf(stderr, "[ERROR] %s: %s\n", what, gx_last_error());
    return rc == GX_EPANIC ? 101 : 1;
}

int run_align(const gx_scores& sc, const std::string& type, const std::string& fasta) {
    Records r;
    load_fasta(fasta, r);
    const size_t nrec = r.size();
    if (nrec < 2) {
        fprintf(stderr, "thread 'main' panicked: index out of bounds: the len is %zu but the index is %zu\n", nrec,
                nrec);
        return 101;  // algo.rs:169 panics on fewer than two sequences
    }
    if (nrec > 2) fprintf(stderr, "[WARN] More than two sequences found. Only the first two will be used.\n");
    fprintf(stderr, "[INFO] Using the following values for scoring:\n[INFO] Match: %lld\n[INFO] Mismatch: %lld\n"
                    "[INFO] Gap: %lld\n[INFO] Opening Gap: %lld\n[INFO] Alignment Type: %s\n",
            (long long)sc.s_match, (long long)sc.s_mismatch, (long long)sc.g, (long long)sc.h, type.c_str());
    const int is_local = (type == "local" || type == "1") ? 1 : 0;  // main.rs:142
    gx_context* ctx = nullptr;
    if (gx_context_create(0, &ctx) != GX_OK) return fail_msg("context", 1);
    const uint8_t* s1 = r.seq(0);
    const uint8_t* s2 = r.seq(1);
    const size_t n = r.sl[0], m = r.sl[1];
    std::vector<gx_step> steps(n + m + 2);
    gx_result res{};
    std::string table_txt;
    if (n < 200 && m < 2000) {
        // small input: keep the planes so that the sequence table can be printed (algo.rs:438)
        gx_table* t = nullptr;
        uint64_t mam = 0;
        int rc = gx_alignment_table(ctx, s1, n, s2, m, &sc, is_local, 0, GX_TABLE_PLANES, &t, &mam);
        if (rc != GX_OK) { gx_context_destroy(ctx); return fail_msg("alignment_table", rc); }
        const size_t cells = (n + 1) * (m + 1);
        std::vector<int64_t> pl(3 * cells);
        for (int k = 0; k < 3 && rc == GX_OK; ++k) rc = gx_table_export_plane(t, k, pl.data() + k * cells, cells, 0);
        if (rc != GX_OK) { gx_table_free(t); gx_context_destroy(ctx); return fail_msg("export", rc); }
        rc = gx_retrace(t, is_local, steps.data(), steps.size(), &res);
        if (rc != GX_OK) { gx_context_destroy(ctx); return fail_msg("retrace", rc); }
        size_t need = 0;
        const int color = stdout_color();
        gx_format_table(s1, n, s2, m, steps.data(), res.n_steps, pl.data(), pl.data() + cells,
                        pl.data() + 2 * cells, color, nullptr, 0, &need);
        table_txt.resize(need);
        rc = gx_format_table(s1, n, s2, m, steps.data(), res.n_steps, pl.data(), pl.data() + cells,
                             pl.data() + 2 * cells, color, table_txt.data(), need, nullptr);
        if (rc != GX_OK) { gx_context_destroy(ctx); return fail_msg("print_alignment_table", rc); }
        table_txt.resize(need ? need - 1 : 0);
    } else {
        int rc = gx_align(ctx, s1, n, s2, m, &sc, is_local, 0, 0, steps.data(), steps.size(), &res);
        if (rc != GX_OK) { gx_context_destroy(ctx); return fail_msg("align", rc); }
        fprintf(stderr, "[WARN] Sequence table too large to visualize\n");
    }
    // (the library logs the table shape, its fill time, the start cell and the
    // retrace lines of algo.rs:175-179, 274-277, 325, 428-436 under GX_LOG=info)
    fputs(table_txt.c_str(), stdout);
    size_t need_txt = 0;
    gx_format_alignment(s1, n, s2, m, steps.data(), res.n_steps, &res, nullptr, 0, &need_txt);
    std::vector<char> txt(need_txt);
    gx_format_alignment(s1, n, s2, m, steps.data(), res.n_steps, &res, txt.data(), txt.size(), nullptr);
    fputs(txt.data(), stdout);
    gx_context_destroy(ctx);
    return 0;
}

// Longest-processing-time partition of `w` over `parts` bins.
std::vector<std::vector<size_t>> lpt(const std::vector<double>& w, int parts) {
    std::vector<size_t> order(w.size());
    for (size_t k = 0; k < w.size(); ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return w[a] > w[b]; });
    std::vector<std::vector<size_t>> bins(parts);
    std::vector<double> load(parts, 0.0);
    for (size_t k : order) {
        int b = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        bins[b].push_back(k);
        load[b] += w[k];
    }
    for (auto& b : bins) std::sort(b.begin(), b.end());
    return bins;
}

int run_all_vs_all(const gx_scores& sc, const std::string& type, const std::string& dir, const std::string& tsv,
                   int ngpu, bool with_self) {
    namespace fs = std::filesystem;
    std::vector<std::string> files;
    std::error_code ec;
    for (const auto& e : fs::directory_iterator(dir, ec))
        if (e.path().extension() == ".fasta") files.push_back(e.path().string());
    if (ec) { fprintf(stderr, "[ERROR] cannot read directory %s: %s\n", dir.c_str(), ec.message().c_str()); return 1; }
    std::sort(files.begin(), files.end());
    fprintf(stderr, "[INFO] Loading sequences from %s\n", dir.c_str());
    Records r;
    for (const auto& f : files) load_fasta(f, r);
    const size_t K = r.size();
    fprintf(stderr, "[INFO] Number of sequences: %zu\n", K);
    const int is_local = (type == "local" || type == "1") ? 1 : 0;
    std::vector<std::pair<size_t, size_t>> pairs;
    for (size_t j = 0; j < K; ++j)
        for (size_t i = 0; i <= j; ++i)
            if (i < j || with_self) pairs.push_back({i, j});
    std::vector<double> w(pairs.size());
    double cells = 0;
    for (size_t p = 0; p < pairs.size(); ++p) {
        w[p] = (double)r.sl[pairs[p].first] * (double)r.sl[pairs[p].second];
        cells += w[p];
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        fprintf(stderr, "[ERROR] no HIP device\n");
        return 1;
    }
    // GX_DEVICE_MAP=d0,d1,...: logical shard g runs on device map[g % len]
    // (e.g. "0,0,0,0" runs a 4-shard plan on one GPU: the multi-GPU code path
    // with several contexts on one device); without it shards clamp to the
    // visible devices
    std::vector<int> devmap;
    if (const char* dm = getenv("GX_DEVICE_MAP"); dm && *dm) {
        for (const char* q = dm; *q;) {
            char* end = nullptr;
            const long d = strtol(q, &end, 10);
            if (end == q) break;
            if (d < 0 || d >= ndev) { fprintf(stderr, "[ERROR] GX_DEVICE_MAP: no HIP device %ld\n", d); return 1; }
            devmap.push_back((int)d);
            q = *end == ',' ? end + 1 : end;
        }
    }
    if (devmap.empty()) {
        if (ngpu <= 0 || ngpu > ndev) ngpu = ndev;
        for (int g = 0; g < ngpu; ++g) devmap.push_back(g);
    } else if (ngpu <= 0) {
        ngpu = (int)devmap.size();
    }
    auto bins = lpt(w, ngpu);
    std::vector<gx_result> res(pairs.size());
    std::vector<int> rcs(ngpu, GX_OK);
    std::vector<std::string> errs(ngpu);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int g = 0; g < ngpu; ++g) {
        th.emplace_back([&, g] {
            const auto& b = bins[g];
            if (b.empty()) return;
            gx_context* ctx = nullptr;
            int rc = gx_context_create(devmap[g % devmap.size()], &ctx);
            if (rc == GX_OK) {
                std::vector<const uint8_t*> a1, a2;
                std::vector<size_t> n1, n2;
                for (size_t p : b) {
                    a1.push_back(r.seq(pairs[p].first)); n1.push_back(r.sl[pairs[p].first]);
                    a2.push_back(r.seq(pairs[p].second)); n2.push_back(r.sl[pairs[p].second]);
                }
                std::vector<gx_result> out(b.size());
                rc = gx_align_batch(ctx, a1.data(), n1.data(), a2.data(), n2.data(), b.size(), &sc, is_local, 0,
                                    nullptr, nullptr, out.data());
                if (rc == GX_OK)
                    for (size_t k = 0; k < b.size(); ++k) res[b[k]] = out[k];
                gx_context_destroy(ctx);
            }
            if (rc != GX_OK) errs[g] = gx_last_error();
            rcs[g] = rc;
        });
    }
    for (auto& t : th) t.join();
    for (int g = 0; g < ngpu; ++g)
        if (rcs[g] != GX_OK) {
            fprintf(stderr, "[ERROR] GPU %d: %s\n", g, errs[g].c_str());
            return rcs[g] == GX_EPANIC ? 101 : 1;
        }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "[INFO] Time taken to compare: %.0f us (%.0f ms), %zu pairs on %d shard(s), %.1f GCUPS\n", us,
            us / 1e3, pairs.size(), ngpu, cells / us / 1e3);
    for (int g = 0; g < ngpu; ++g) {
        double cg = 0;
        for (size_t p : bins[g]) cg += w[p];
        fprintf(stderr, "[INFO] shard %d: device %d, %zu pairs, %.3g cells\n", g, devmap[g % devmap.size()],
                bins[g].size(), cg);
    }
    // matrix in the reference's layout: row j, column i filled for i <= j (main.rs:253-264)
    std::vector<const gx_result*> cellp(K * K, nullptr);
    for (size_t p = 0; p < pairs.size(); ++p) cellp[pairs[p].second * K + pairs[p].first] = &res[p];
    FILE* f = fopen(tsv.c_str(), "w");
    if (!f) { fprintf(stderr, "[ERROR] cannot write %s\n", tsv.c_str()); return 1; }
    auto table = [&](FILE* o, bool header_blank, auto field) {
        fprintf(o, header_blank ? " \t" : "\t");
        for (size_t i = 0; i < K; ++i) fprintf(o, "%zu\t", i);
        fprintf(o, "\n");
        for (size_t j = 0; j < K; ++j) {
            fprintf(o, "%zu\t", j);
            for (size_t i = 0; i < K; ++i) {
                const gx_result* c = cellp[j * K + i];
                fprintf(o, "%lld\t", c ? (long long)field(*c) : 0LL);
            }
            fprintf(o, "\n");
        }
    };
    table(f, false, [](const gx_result& c) { return c.score; });
    fclose(f);
    printf("Similarity TSV:\n");
    table(stdout, true, [](const gx_result& c) { return c.score; });
    printf("\nMatches TSV:\n");
    table(stdout, true, [](const gx_result& c) { return (int64_t)c.matches; });
    printf("\nSequences:\n");
    for (size_t k = 0; k < K; ++k) printf("%zu\t%s\t%llu\n", k, r.name(k).c_str(), (unsigned long long)r.sl[k]);
    return 0;
}

// Command::Compare (main.rs:216-379) on GPU 0.
int run_compare(const std::string& dir, const std::string& tsv) {
    namespace fs = std::filesystem;
    std::vector<std::string> files;
    std::error_code ec;
    for (const auto& e : fs::directory_iterator(dir, ec))
        if (e.path().extension() == ".fasta") files.push_back(e.path().string());
    if (ec) { fprintf(stderr, "[ERROR] cannot read directory %s: %s\n", dir.c_str(), ec.message().c_str()); return 1; }
    std::sort(files.begin(), files.end());
    const char* lg = getenv("GX_LOG");
    const bool info = lg && (!strcmp(lg, "info") || !strcmp(lg, "debug"));
    if (info) fprintf(stderr, "[INFO] MODE: Compare\n[INFO] FASTA directory: %s\n[INFO] Loading sequences from %s\n",
                      dir.c_str(), dir.c_str());
    Records r;
    for (const auto& f : files) load_fasta(f, r);
    const size_t K = r.size();
    if (info) fprintf(stderr, "[INFO] Number of sequences: %zu\n", K);
    gx_context* ctx = nullptr;
    if (gx_context_create(0, &ctx) != GX_OK) return fail_msg("context", 1);
    std::vector<const uint8_t*> seqs(K);
    std::vector<size_t> lens(K);
    for (size_t k = 0; k < K; ++k) { seqs[k] = r.seq(k); lens[k] = r.sl[k]; }
    std::vector<gx_compare_cell> mat(K * K);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = gx_compare_matrix(ctx, seqs.data(), lens.data(), K, mat.data());
    const auto us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    if (rc != GX_OK) { gx_context_destroy(ctx); return fail_msg("compare", rc); }
    if (info) {
        uint64_t ng = 0, nh = 0, no = 0, nl = 0;
        gx_compare_info(ctx, &ng, &nh, &no, &nl);
        fprintf(stderr, "[INFO] [FindPath] Time taken to compare: %lld us (%lld ms)\n", (long long)us,
                (long long)(us / 1000));
        fprintf(stderr, "[INFO] %llu sub-problems on the GPU in %llu levels, %llu on the host (%llu overflowed)\n",
                (unsigned long long)ng, (unsigned long long)nl, (unsigned long long)nh, (unsigned long long)no);
    }
    gx_context_destroy(ctx);
    FILE* f = fopen(tsv.c_str(), "w");
    if (!f) { fprintf(stderr, "[ERROR] cannot write %s\n", tsv.c_str()); return 1; }
    // main.rs:337-378: the file and the first stdout block carry the score, the second block first_lcs_length
    auto table = [&](FILE* o, bool header_blank, bool lcs) {
        fprintf(o, header_blank ? " \t" : "\t");
        for (size_t i = 0; i < K; ++i) fprintf(o, "%zu\t", i);
        fprintf(o, "\n");
        for (size_t j = 0; j < K; ++j) {
            fprintf(o, "%zu\t", j);
            for (size_t i = 0; i < K; ++i) {
                const gx_compare_cell& c = mat[j * K + i];
                fprintf(o, "%llu\t", (unsigned long long)(lcs ? c.first_lcs : c.score));
            }
            fprintf(o, "\n");
        }
    };
    table(f, false, false);
    fclose(f);
    printf("Similarity TSV:\n");
    table(stdout, true, false);
    printf("\nLCS Length TSV:\n");
    table(stdout, true, true);
    return 0;
}

// Command::SuffixTree (main.rs:154-215) on GPU 0: the BWT and the statistics
// of the first record's suffix tree, from its suffix array.
int run_suffix_tree(const std::string& fasta, const std::string& alphabet, bool stats, std::string bwt_path) {
    namespace fs = std::filesystem;
    const char* lg = getenv("GX_LOG");
    const bool info = lg && (!strcmp(lg, "info") || !strcmp(lg, "debug"));
    if (info) fprintf(stderr, "[INFO] MODE: Suffix Tree\n[INFO] Loading sequences from %s\n", fasta.c_str());
    Records r;
    load_fasta(fasta, r);
    if (!r.size()) {
        fprintf(stderr, "thread 'main' panicked: index out of bounds: the len is 0 but the index is 0\n");
        return 101;  // main.rs:168 indexes sequences[0]
    }
    const uint8_t* s = r.seq(0);
    const size_t n = r.sl[0];
    if (!alphabet.empty()) {
        // SuffixTree::new (tree.rs:138-148) and get_child_index (tree.rs:56-63)
        FILE* f = fopen(alphabet.c_str(), "rb");
        if (!f) { fprintf(stderr, "thread 'main' panicked: Could not read alphabet file: %s\n", alphabet.c_str()); return 101; }
        bool in[256] = {};
        for (const char* q = "$!@#%^&*()-_=+{}[]|;:'<>,.?/~` \n"; *q; ++q) in[(uint8_t)*q] = true;   // STRING_TERMINATORS
        for (int c; (c = fgetc(f)) != EOF;) in[c & 255] = true;
        fclose(f);
        for (size_t k = 0; k < n; ++k)
            if (!in[s[k]]) {
                fprintf(stderr, "thread 'main' panicked: Character %c not found in alphabet\n", s[k]);
                return 101;
            }
    }
    gx_context* ctx = nullptr;
    if (gx_context_create(0, &ctx) != GX_OK) return fail_msg("context", 1);
    gx_suffix_stats st{};
    std::vector<uint8_t> bwt(n + 1);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = gx_suffix_tree_stats(ctx, s, n, &st, bwt.data(), nullptr, nullptr);
    const auto us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    if (rc != GX_OK) { gx_context_destroy(ctx); return fail_msg("suffix-tree", rc); }
    if (info) {
        uint64_t rounds = 0, passes = 0;
        gx_suffix_info(ctx, &rounds, &passes, nullptr, nullptr, nullptr);
        fprintf(stderr, "[INFO] [FindPath] Time taken to build suffix tree: %lld us (%lld ms)\n", (long long)us,
                (long long)(us / 1000));
        fprintf(stderr, "[INFO] suffix array of %zu suffixes: %llu doubling rounds, %llu radix passes\n", n + 1,
                (unsigned long long)rounds, (unsigned long long)passes);
    }
    gx_context_destroy(ctx);
    if (!stats) return 0;
    if (bwt_path.empty()) {
        // main.rs:181-191: the file name behind the last '/' and '\\', without ".fasta"
        std::string name = fasta.substr(fasta.find_last_of('/') == std::string::npos ? 0 : fasta.find_last_of('/') + 1);
        name = name.substr(name.find_last_of('\\') == std::string::npos ? 0 : name.find_last_of('\\') + 1);
        for (size_t p; (p = name.find(".fasta")) != std::string::npos;) name.erase(p, 6);
        bwt_path = "BWT_out/" + name + "_bwt.txt";
    }
    if (info) fprintf(stderr, "[INFO] BWT Path: %s\n", bwt_path.c_str());
    std::error_code ec;
    if (fs::path(bwt_path).has_parent_path()) fs::create_directories(fs::path(bwt_path).parent_path(), ec);
    FILE* f = fopen(bwt_path.c_str(), "w");
    if (!f) { fprintf(stderr, "[ERROR] cannot write %s\n", bwt_path.c_str()); return 1; }
    std::string lines(2 * bwt.size(), '\n');   // main.rs:207-211: one character per line
    for (size_t k = 0; k < bwt.size(); ++k) lines[2 * k] = (char)bwt[k];
    fwrite(lines.data(), 1, lines.size(), f);
    fclose(f);
    size_t need = 0;
    gx_format_suffix_stats(&st, bwt.data(), bwt.size(), nullptr, 0, &need);
    std::vector<char> txt(need);
    if (gx_format_suffix_stats(&st, bwt.data(), bwt.size(), txt.data(), txt.size(), nullptr) != GX_OK)
        return fail_msg("stats", 1);
    printf("\nStats: %s\n", txt.data());   // display.rs:54 (the Graphviz block is out of scope)
    return 0;
}

// Search mode on GPU 0 (no counterpart in the reference): every record of the
// pattern file against the suffix index of the genome's first record.
// -k K: at most K substitutions (gx_suffix_index_search_approx); -e K: at most K
// differences (gx_suffix_index_search_edit); both below 0: exact.  sc (with -e alone): the
// reported windows are aligned under these scores on the band of K (gx_suffix_index_extend).
// strands: 0 without --strands (the forward strand, lines as they always were), else GX_STRAND_*: a line per item of
// the item batch, '+' or '-' behind the name.
int run_search(const std::string& fasta, const std::string& patterns, uint32_t max_hits, const std::string& out_path,
               int kmis, int kedit, const gx_scores* sc, uint32_t strands) {
    const char* lg = getenv("GX_LOG");
    const bool info = lg && (!strcmp(lg, "info") || !strcmp(lg, "debug"));
    if (info) fprintf(stderr, "[INFO] MODE: Search\n[INFO] Loading sequences from %s and %s\n", fasta.c_str(), patterns.c_str());
    Records g, q;
    load_fasta(fasta, g);
    load_fasta(patterns, q);
    if (!g.size()) { fprintf(stderr, "[ERROR] no record in %s\n", fasta.c_str()); return 1; }
    const size_t ncall = q.size();
    const uint32_t st = strands ? strands : GX_STRAND_FWD;
    const size_t npat = ncall * (st == GX_STRAND_BOTH ? 2 : 1);   // the items
    std::vector<uint8_t> packed;
    std::vector<uint64_t> off(ncall + 1, 0);
    for (size_t p = 0; p < ncall; ++p) {
        packed.insert(packed.end(), q.seq(p), q.seq(p) + q.sl[p]);
        off[p + 1] = packed.size();
    }
    gx_context* ctx = nullptr;
    if (gx_context_create(0, &ctx) != GX_OK) return fail_msg("context", 1);
    gx_suffix_index* idx = nullptr;
    auto t0 = std::chrono::steady_clock::now();
    int rc = gx_suffix_index_build(ctx, g.seq(0), g.sl[0], &idx);
    if (rc != GX_OK) { gx_context_destroy(ctx); return fail_msg("search: index", rc); }
    const auto build_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    const bool exact = kmis < 0 && kedit < 0;
    std::vector<gx_search_hit> hits(exact ? npat : 0);
    std::vector<gx_approx_hit> ahits(kmis < 0 ? 0 : npat);
    std::vector<gx_edit_hit> ehits(kedit < 0 ? 0 : npat);
    std::vector<uint64_t> hoff(npat + 1, 0);
    std::vector<uint32_t> pos(std::max<size_t>(1, npat * (size_t)std::min<uint64_t>(max_hits, 16)));
    std::vector<uint8_t> dst(exact ? 0 : pos.size());
    std::vector<uint32_t> sta(kedit < 0 ? 0 : pos.size());
    t0 = std::chrono::steady_clock::now();
    for (int pass = 0; pass < 2; ++pass) {   // GX_ECAP: hit_offsets is complete; allocate and repeat
        if (exact)
            rc = gx_suffix_index_search_strands(idx, packed.data(), off.data(), ncall, st, hits.data(), max_hits,
                                                max_hits ? pos.data() : nullptr, pos.size(), max_hits ? hoff.data() : nullptr);
        else if (kedit >= 0)
            rc = gx_suffix_index_search_edit_strands(idx, packed.data(), off.data(), ncall, st, (uint32_t)kedit, ehits.data(),
                                                     max_hits, max_hits ? pos.data() : nullptr, max_hits ? dst.data() : nullptr,
                                                     max_hits ? sta.data() : nullptr, pos.size(),
                                                     max_hits ? hoff.data() : nullptr);
        else
            rc = gx_suffix_index_search_approx_strands(idx, packed.data(), off.data(), ncall, st, (uint32_t)kmis, ahits.data(),
                                                       max_hits, max_hits ? pos.data() : nullptr,
                                                       max_hits ? dst.data() : nullptr, pos.size(),
                                                       max_hits ? hoff.data() : nullptr);
        if (rc != GX_ECAP) break;
        pos.assign((size_t)hoff[npat], 0);
        if (!exact) dst.assign((size_t)hoff[npat], 0);
        if (kedit >= 0) sta.assign((size_t)hoff[npat], 0);
    }
    const auto us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    std::vector<gx_extend_hit> xhits;
    std::vector<uint64_t> coff;
    std::vector<uint32_t> cig;
    if (rc == GX_OK && sc && max_hits) {   // the counts and the offsets first, then the exact capacity
        t0 = std::chrono::steady_clock::now();
        xhits.resize((size_t)hoff[npat] + 1);
        coff.assign((size_t)hoff[npat] + 1, 0);
        rc = gx_suffix_index_extend_strands(idx, packed.data(), off.data(), ncall, st, hoff.data(), sta.data(), pos.data(), sc,
                                            (uint32_t)kedit, xhits.data(), nullptr, 0, coff.data());
        if (rc == GX_OK) {
            cig.resize((size_t)coff.back() + 1);
            rc = gx_suffix_index_extend_strands(idx, packed.data(), off.data(), ncall, st, hoff.data(), sta.data(), pos.data(),
                                                sc, (uint32_t)kedit, xhits.data(), cig.data(), cig.size(), coff.data());
        }
        const auto xus = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        if (rc == GX_OK && info) {
            uint64_t xh = 0, cells = 0, tb = 0, chunks = 0;
            double fms = 0, wms = 0;
            gx_extend_info(ctx, &xh, &cells, &tb, &chunks, &fms, &wms);
            fprintf(stderr, "[INFO] %llu hits aligned on the band of %d in %lld us (%llu cell updates, %llu trace bytes in %llu "
                            "chunks, fill %.3f ms, walk %.3f ms)\n",
                    (unsigned long long)xh, kedit, (long long)xus, (unsigned long long)cells, (unsigned long long)tb,
                    (unsigned long long)chunks, fms, wms);
        }
    }
    if (rc == GX_OK && info && kedit >= 0) {
        uint64_t cands = 0, pre = 0, cells = 0;
        double sms = 0, vms = 0, dms = 0;
        gx_edit_info(ctx, &cands, &pre, &cells, &sms, &vms, &dms);
        fprintf(stderr, "[INFO] index of %llu bases built in %lld us; %zu patterns searched with at most %d differences in "
                        "%lld us (%llu candidates, %llu ends before dedupe, %llu cell updates, seeds %.3f ms, verify %.3f ms, "
                        "dedupe %.3f ms)\n",
                (unsigned long long)g.sl[0], (long long)build_us, npat, kedit, (long long)us, (unsigned long long)cands,
                (unsigned long long)pre, (unsigned long long)cells, sms, vms, dms);
    } else if (rc == GX_OK && info && kmis >= 0) {
        uint64_t cands = 0, words = 0;
        double sms = 0, vms = 0;
        gx_approx_info(ctx, &cands, &words, &sms, &vms);
        fprintf(stderr, "[INFO] index of %llu bases built in %lld us; %zu patterns searched with at most %d mismatches in "
                        "%lld us (%llu candidates, %llu word compares, seeds %.3f ms, verify %.3f ms)\n",
                (unsigned long long)g.sl[0], (long long)build_us, npat, kmis, (long long)us, (unsigned long long)cands,
                (unsigned long long)words, sms, vms);
    } else if (rc == GX_OK && info) {
        uint64_t words = 0;
        double sms = 0, lms = 0;
        gx_search_info(ctx, &words, &sms, &lms);
        fprintf(stderr, "[INFO] index of %llu bases built in %lld us; %zu patterns searched in %lld us "
                        "(%llu word compares, interval kernel %.3f ms, locate %.3f ms)\n",
                (unsigned long long)g.sl[0], (long long)build_us, npat, (long long)us, (unsigned long long)words, sms, lms);
    }
    gx_suffix_index_free(idx);
    gx_context_destroy(ctx);
    if (rc != GX_OK) return fail_msg("search", rc);
    FILE* f = out_path.empty() ? stdout : fopen(out_path.c_str(), "w");
    if (!f) { fprintf(stderr, "[ERROR] cannot write %s\n", out_path.c_str()); return 1; }
    for (size_t p = 0; p < npat; ++p) {
        // (item p is record p % ncall, on the - strand in the reverse items; the strand column only with --strands)
        const size_t c = p % ncall;
        const std::string name = q.name(c) + (strands ? (st == GX_STRAND_REV || p >= ncall ? "\t-" : "\t+") : "");
        if (kedit >= 0) {   // name, length, count, best_dist, best_end, start-end:dist triples
            fprintf(f, "%s\t%llu\t%u\t%u\t%u\t", name.c_str(), (unsigned long long)q.sl[c], ehits[p].count,
                    ehits[p].best_dist, ehits[p].best_end);
            for (uint64_t k = hoff[p]; k < hoff[p + 1]; ++k) {
                fprintf(f, k == hoff[p] ? "%u-%u:%u" : ",%u-%u:%u", sta[k], pos[k], (unsigned)dst[k]);
                if (xhits.empty()) continue;
                fprintf(f, ":%d:", xhits[k].score);   // start-end:dist:score:CIGAR
                for (uint64_t r = coff[k]; r < coff[k + 1]; ++r) fprintf(f, "%u%c", cig[r] >> 4, "MID?"[cig[r] & 3u]);
            }
        } else if (exact) {
            fprintf(f, "%s\t%llu\t%u\t%u\t%u\t", name.c_str(), (unsigned long long)q.sl[c], hits[p].count,
                    hits[p].prefix_len, hits[p].prefix_pos);
            for (uint64_t k = hoff[p]; k < hoff[p + 1]; ++k) fprintf(f, k == hoff[p] ? "%u" : ",%u", pos[k]);
        } else {   // name, length, count, best_dist, best_pos, pos:dist pairs
            fprintf(f, "%s\t%llu\t%u\t%u\t%u\t", name.c_str(), (unsigned long long)q.sl[c], ahits[p].count,
                    ahits[p].best_dist, ahits[p].best_pos);
            for (uint64_t k = hoff[p]; k < hoff[p + 1]; ++k)
                fprintf(f, k == hoff[p] ? "%u:%u" : ",%u:%u", pos[k], (unsigned)dst[k]);
        }
        fputc('\n', f);
    }
    if (f != stdout) fclose(f);
    return 0;
}

// search --mem L on GPU 0: the MEMs of every record of the query file against the genome's first record.
// chain: with --chain, the parameters of gx_chain_anchors on those MEMs; the file then holds the chains.
// strands: as for run_search; with --strands the query length follows the strand column, so that a reader can map
// a - item's qpos back: the same bases begin at length - qpos - len in the record.
int run_mems(const std::string& fasta, const std::string& queries, uint32_t min_len, const std::string& out_path,
             const gx_chain_params* chain, uint32_t strands) {
    const char* lg = getenv("GX_LOG");
    const bool info = lg && (!strcmp(lg, "info") || !strcmp(lg, "debug"));
    if (info) fprintf(stderr, "[INFO] MODE: Search (MEMs)\n[INFO] Loading sequences from %s and %s\n", fasta.c_str(), queries.c_str());
    Records g, q;
    load_fasta(fasta, g);
    load_fasta(queries, q);
    if (!g.size()) { fprintf(stderr, "[ERROR] no record in %s\n", fasta.c_str()); return 1; }
    const size_t ncall = q.size();
    const uint32_t st = strands ? strands : GX_STRAND_FWD;
    const size_t nq = ncall * (st == GX_STRAND_BOTH ? 2 : 1);   // the items
    std::vector<uint8_t> packed;
    std::vector<uint64_t> off(ncall + 1, 0), moff(nq + 1, 0), cand(nq + 1, 0);
    for (size_t c = 0; c < ncall; ++c) {
        packed.insert(packed.end(), q.seq(c), q.seq(c) + q.sl[c]);
        off[c + 1] = packed.size();
    }
    gx_context* ctx = nullptr;
    if (gx_context_create(0, &ctx) != GX_OK) return fail_msg("context", 1);
    gx_suffix_index* idx = nullptr;
    auto t0 = std::chrono::steady_clock::now();
    int rc = gx_suffix_index_build(ctx, g.seq(0), g.sl[0], &idx);
    if (rc != GX_OK) { gx_context_destroy(ctx); return fail_msg("search: index", rc); }
    const auto build_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    std::vector<gx_mem> mems;
    t0 = std::chrono::steady_clock::now();
    // the counts first, then the exact capacity
    rc = gx_suffix_index_mems_strands(idx, packed.data(), off.data(), ncall, st, min_len, nullptr, 0, moff.data(), cand.data());
    if (rc == GX_OK && moff[nq]) {
        mems.resize((size_t)moff[nq]);
        rc = gx_suffix_index_mems_strands(idx, packed.data(), off.data(), ncall, st, min_len, mems.data(), mems.size(), moff.data(),
                                          cand.data());
    }
    const auto us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    if (rc == GX_OK && info) {
        uint64_t cands = 0, kept = 0, words = 0;
        double tms = 0, sms = 0, ems = 0;
        gx_match_info(ctx, &cands, &kept, &words, &tms, &sms, &ems);
        fprintf(stderr, "[INFO] index of %llu bases built in %lld us; %zu queries of %llu bases matched at min_len %u in %lld us "
                        "(%llu candidates, %llu MEMs, %llu word compares, seeds %.3f ms, emit %.3f ms)\n",
                (unsigned long long)g.sl[0], (long long)build_us, nq, (unsigned long long)(off[ncall] * (nq / std::max<size_t>(ncall, 1))), min_len, (long long)us,
                (unsigned long long)cands, (unsigned long long)kept, (unsigned long long)words, sms, ems);
    }
    gx_suffix_index_free(idx);
    // --chain: one call, since chains and members are at most the anchors; above 2^22 anchors that many are
    // asked for first, and a GX_ECAP, which leaves the totals, is answered with the exact capacities
    std::vector<gx_chain> chains;
    std::vector<uint32_t> members;
    std::vector<uint64_t> coff(nq + 1, 0);
    const int mems_rc = rc;
    if (rc == GX_OK && chain) {
        uint64_t mtot = 0;
        t0 = std::chrono::steady_clock::now();
        chains.resize(std::min<size_t>(std::max<size_t>(mems.size(), 1), (size_t)1 << 22));
        members.resize(chains.size());
        for (int attempt = 0; attempt < 2; ++attempt) {
            rc = gx_chain_anchors(ctx, mems.data(), moff.data(), nq, chain, nullptr, nullptr, chains.data(), chains.size(),
                                  members.data(), members.size(), coff.data(), &mtot);
            if (rc != GX_ECAP) break;
            chains.resize((size_t)coff[nq]);
            members.resize((size_t)mtot);
        }
        const auto cus = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        if (rc == GX_OK && info) {
            uint64_t an = 0, segs = 0, evals = 0, nch = 0;
            double sms = 0, cms = 0;
            gx_chain_info(ctx, &an, &segs, &evals, &nch, &sms, &cms);
            fprintf(stderr, "[INFO] %llu anchors in %llu segments chained in %lld us (%llu pair evaluations, %llu chains, "
                            "score %.3f ms, chains %.3f ms)\n",
                    (unsigned long long)an, (unsigned long long)segs, (long long)cus, (unsigned long long)evals,
                    (unsigned long long)nch, sms, cms);
        }
    }
    gx_context_destroy(ctx);
    if (rc != GX_OK) return fail_msg(mems_rc != GX_OK ? "search --mem" : "search --chain", rc);
    FILE* f = out_path.empty() ? stdout : fopen(out_path.c_str(), "w");
    if (!f) { fprintf(stderr, "[ERROR] cannot write %s\n", out_path.c_str()); return 1; }
    // an item's name: its record's, and with --strands the strand and the record's length behind it
    auto name_of = [&](size_t c) {
        std::string s = q.name(c % ncall);
        if (strands) s += (st == GX_STRAND_REV || c >= ncall ? "\t-\t" : "\t+\t") + std::to_string(q.sl[c % ncall]);
        return s;
    };
    if (chain) {
        for (size_t c = 0; c < nq; ++c)
            for (uint64_t k = coff[c]; k < coff[c + 1]; ++k)
                fprintf(f, "%s\t%llu\t%d\t%u\t%u\t%u\t%u\t%u\n", name_of(c).c_str(), (unsigned long long)(k - coff[c]),
                        chains[k].score, chains[k].n_anchors, chains[k].qstart, chains[k].qend, chains[k].tstart, chains[k].tend);
        for (size_t c = 0; c < nq; ++c)
            if (coff[c + 1] == coff[c]) fprintf(f, "%s\t-\t0\n", name_of(c).c_str());
        if (f != stdout) fclose(f);
        return 0;
    }
    for (size_t c = 0; c < nq; ++c)
        for (uint64_t k = moff[c]; k < moff[c + 1]; ++k)
            fprintf(f, "%s\t%u\t%u\t%u\n", name_of(c).c_str(), mems[k].qpos, mems[k].tpos, mems[k].len);
    for (size_t c = 0; c < nq; ++c)
        if (moff[c + 1] == moff[c]) fprintf(f, "%s\t-\t-\t0\n", name_of(c).c_str());
    if (f != stdout) fclose(f);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    // main.rs:91-96: the CLI logs at info unless told otherwise
    setenv("GX_LOG", getenv("GX_LOG") ? getenv("GX_LOG") : "info", 1);
    std::string config = "config.toml", type, fasta, dir, tsv = "similarity_matrix.tsv", mode, patterns;
    int ngpu = 0;
    uint32_t strands = 0;   // (0: no --strands)
    long long max_hits = 16, kmis = -1, kedit = -1, mem_len = -1;
    bool with_self = true, stats = false, out_set = false, cigar = false, chain = false, chain_opt = false;
    gx_chain_params cp{GX_CHAIN_DEFAULT_W_MATCH,  GX_CHAIN_DEFAULT_W_DRIFT,  GX_CHAIN_DEFAULT_MAX_GAP,
                       GX_CHAIN_DEFAULT_MAX_DRIFT, GX_CHAIN_DEFAULT_MAX_PRED, GX_CHAIN_DEFAULT_MIN_SCORE};
    // a chain parameter's number: the library holds it to its range
    auto chain_num = [&](long long& dst, const std::string& v) {
        char* end = nullptr;
        dst = strtoll(v.c_str(), &end, 10);
        chain_opt = true;
        return end != v.c_str() && !*end && dst >= 0 && dst <= 0x7FFFFFFFll;
    };
    for (int k = 1; k < argc; ++k) {
        std::string a = argv[k];
        auto next = [&](std::string& dst) {
            if (k + 1 >= argc) { usage(); exit(2); }
            dst = argv[++k];
        };
        if (a == "-c" || a == "--config-path") next(config);
        else if (a == "align" || a == "all-vs-all" || a == "compare" || a == "suffix-tree" || a == "search") mode = a;
        else if (a == "-a" || a == "--alignment-type" || a == "--alphabet-file") next(type);   // (suffix-tree: the alphabet)
        else if (a == "-f" || a == "--fasta-path") next(fasta);
        else if (a == "-d" || a == "--fasta-dir") next(dir);
        else if (a == "-o" || a == "--output") { next(tsv); out_set = true; }
        else if (a == "--stats") stats = true;
        else if (a == "-p" || a == "--patterns") next(patterns);
        else if (a == "--max-hits") { std::string v; next(v); max_hits = atoll(v.c_str()); }
        else if (a == "-k" || a == "--mismatches") { std::string v; next(v); kmis = atoll(v.c_str()); if (kmis < 0) { usage(); return 2; } }
        else if (a == "-e" || a == "--edits") { std::string v; next(v); kedit = atoll(v.c_str()); if (kedit < 0) { usage(); return 2; } }
        else if (a == "--cigar") cigar = true;
        else if (a == "--mem") { std::string v; next(v); mem_len = atoll(v.c_str()); if (mem_len < 1 || mem_len > 0xFFFFFFFFll) { usage(); return 2; } }
        else if (a == "--chain") chain = true;
        else if (a == "--strands") {
            std::string v;
            next(v);
            strands = v == "forward" ? GX_STRAND_FWD : v == "reverse" ? GX_STRAND_REV : v == "both" ? GX_STRAND_BOTH : 0;
            if (!strands) { usage(); return 2; }
        }
        else if (a == "--chain-gap" || a == "--chain-drift" || a == "--chain-pred" || a == "--chain-min-score") {
            std::string v;
            long long x = 0;
            next(v);
            if (!chain_num(x, v)) { usage(); return 2; }
            if (a == "--chain-gap") cp.max_gap = (uint32_t)x;
            else if (a == "--chain-drift") cp.max_drift = (uint32_t)x;
            else if (a == "--chain-pred") cp.max_pred = (uint32_t)x;
            else cp.min_score = (int32_t)x;
        }
        else if (a == "--suffix-links") {}   // (the reference's build strategy: no counterpart)
        else if (a == "-g" || a == "--gpus") { std::string v; next(v); ngpu = atoi(v.c_str()); }
        else if (a == "--no-self") with_self = false;
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else { usage(); return 2; }
    }
    const bool by_file = mode == "align" || mode == "suffix-tree" || mode == "search";
    if (mode.empty() || (by_file && fasta.empty()) || (!by_file && dir.empty()) ||
        (mode == "search" && (patterns.empty() || max_hits < 0 || max_hits > 0xFFFFFFFFll || kmis > 0xFFFF || kedit > 0xFFFF ||
                              (kmis >= 0 && kedit >= 0) || (mem_len >= 0 && (kmis >= 0 || kedit >= 0)))) ||
        (cigar && (mode != "search" || kedit < 0)) || (chain && (mode != "search" || mem_len < 0)) || (chain_opt && !chain) ||
        (strands && mode != "search")) {
        usage();
        return 2;
    }
    if (mode == "compare") return run_compare(dir, tsv);   // (reads no scores: main.rs:216-221)
    if (mode == "search" && mem_len >= 0) return run_mems(fasta, patterns, (uint32_t)mem_len, out_set ? tsv : std::string(), chain ? &cp : nullptr, strands);
    if (mode == "search" && !cigar)
        return run_search(fasta, patterns, (uint32_t)max_hits, out_set ? tsv : std::string(), (int)kmis, (int)kedit, nullptr, strands);
    if (mode == "suffix-tree") return run_suffix_tree(fasta, type, stats, out_set ? tsv : std::string());
    gx_scores sc;
    if (gx_config_load(config.c_str(), &sc) != GX_OK) {
        fprintf(stderr, "[ERROR] %s\n", gx_last_error());
        return 1;  // config.rs: exit(1)
    }
    if (mode == "search") return run_search(fasta, patterns, (uint32_t)max_hits, out_set ? tsv : std::string(), -1, (int)kedit, &sc, strands);
    if (mode == "align") return run_align(sc, type.empty() ? "local" : type, fasta);  // main.rs:35 default "local"
    return run_all_vs_all(sc, type.empty() ? "global" : type, dir, tsv, ngpu, with_self);
}
