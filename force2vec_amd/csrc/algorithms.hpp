// algorithms.hpp -- host-side mirror of the reference's `class algorithms`
// (sample/algorithms.h:51-137) over the C ABI of libf2v: same constructor arguments, same
// method names and argument meaning for the options 5-11 entry points, same side effects
// (the "... Wall time required:" line, the .embd file, result = {seconds}).  The embedding
// matrix lives in HBM; nothing here computes forces.
#ifndef F2V_ALGORITHMS_HPP_
#define F2V_ALGORITHMS_HPP_
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "f2v.h"

#define VALUETYPE float
#define INDEXTYPE unsigned int

namespace f2v_host {

struct CSRGraph {  // CSR<INDEXTYPE, VALUETYPE> of sample/CSR.h:89-96 (values are never read by options 5-11)
    INDEXTYPE rows = 0;
    uint64_t nnz = 0;
    INDEXTYPE *rowptr = nullptr;
    INDEXTYPE *colids = nullptr;
    ~CSRGraph() { f2v_free(rowptr); f2v_free(colids); }
    CSRGraph() = default;
    CSRGraph(const CSRGraph &) = delete;
    CSRGraph &operator=(const CSRGraph &) = delete;
};

// SetInputMatricesAsCSR, sample/commonutility.h:44-54.  `use_cache`: keep / reuse "<input>.f2vcsr", the binary
// CSR of the parsed file (the same arrays, so training is bit-identical); an input that already ends in
// ".f2vcsr" is read as such.
inline void SetInputMatricesAsCSR(CSRGraph &A, const std::string &inputfile, bool use_cache = false) {
    const std::string ext = ".f2vcsr";
    const bool is_bin = inputfile.size() > ext.size() && inputfile.compare(inputfile.size() - ext.size(), ext.size(), ext) == 0;
    const std::string cache = is_bin ? inputfile : inputfile + ext;
    if (is_bin || use_cache) {
        if (f2v_read_csr_bin(cache.c_str(), &A.rows, &A.nnz, &A.rowptr, &A.colids) == F2V_OK) {
            std::cout << "Reading binary CSR cache:" << cache << std::endl;
            std::cout << "Input Matrix: Rows = " << A.rows << ", nnz = " << A.nnz << std::endl;
            return;
        }
        if (is_bin) throw std::runtime_error(f2v_last_error());
    }
    std::cout << "Reading input matrices in text (ascii)... " << std::endl;
    std::cout << "Input File Directory:" << inputfile << std::endl;
    if (f2v_read_mtx(inputfile.c_str(), &A.rows, &A.nnz, &A.rowptr, &A.colids) != F2V_OK) throw std::runtime_error(f2v_last_error());
    std::cout << "Input Matrix: Rows = " << A.rows << ", nnz = " << A.nnz << std::endl;
    if (use_cache && f2v_write_csr_bin(cache.c_str(), A.rowptr, A.colids, A.rows, A.nnz) != F2V_OK)
        std::cerr << "warning: " << f2v_last_error() << std::endl;
}

// -holdout <f>: the input graph split by f2v_edge_split(frac, seed, ratio) -- with -holdout-keep forest by f2v_edge_split_connected -- on `device` -- the training graph (the run's handle is
// created on it), the hidden edges and as many non-edges of the full graph per vertex.  The split needs no embeddings: it runs on a
// handle of its own, gone before the training handle is made.
struct Holdout {
    CSRGraph train;
    std::vector<uint32_t> held_u, held_v, neg_u, neg_v;
};
inline void SplitForHoldout(const CSRGraph &A, double frac, uint32_t ratio, uint64_t seed, int device, Holdout &out, bool forest = false) {
    // -holdout-keep forest: f2v_edge_split_connected, the same call but for what it protects
    const auto split_call = forest ? f2v_edge_split_connected : f2v_edge_split;
    f2v_handle h = nullptr;
    if (f2v_create(A.rowptr, A.colids, A.rows, A.nnz, 1, device, &h) != F2V_OK) throw std::runtime_error(f2v_last_error());
    uint64_t nnz = 0, held = 0, neg = 0;
    int rc = split_call(h, frac, seed, ratio, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, &nnz, &held, &neg, nullptr);
    if (rc == F2V_OK) {
        out.train.rows = A.rows;
        out.train.nnz = nnz;
        out.train.rowptr = static_cast<INDEXTYPE *>(malloc(((size_t)A.rows + 1) * sizeof(INDEXTYPE)));
        out.train.colids = static_cast<INDEXTYPE *>(malloc((nnz ? nnz : 1) * sizeof(INDEXTYPE)));
        out.held_u.resize(held + 1);  // (+ 1: an empty vector has no array to name)
        out.held_v.resize(held + 1);
        out.neg_u.resize(neg + 1);
        out.neg_v.resize(neg + 1);
        rc = out.train.rowptr && out.train.colids
                 ? split_call(h, frac, seed, ratio, out.train.rowptr, out.train.colids, nnz ? nnz : 1, out.held_u.data(), out.held_v.data(), held + 1,
                                  out.neg_u.data(), out.neg_v.data(), neg + 1, &nnz, &held, &neg, nullptr)
                 : F2V_ENOMEM;
        for (auto *a : {&out.held_u, &out.held_v}) a->resize(held);
        for (auto *a : {&out.neg_u, &out.neg_v}) a->resize(neg);
    }
    const std::string why = rc == F2V_OK ? "" : rc == F2V_ENOMEM ? "out of memory" : f2v_last_error();
    f2v_destroy(h);
    if (rc != F2V_OK) throw std::runtime_error(why);
    std::cout << "Holdout: " << held << " of the edges hidden, " << neg << " non-edges drawn, training graph nnz = " << nnz << std::endl;
}

class algorithms {
   public:
    f2v_handle h = nullptr;
    INDEXTYPE DIM, rows;
    std::string filename, outputdir;
    double gpu_train_seconds = 0.0;  // device time of the epoch loop alone
    bool binary_output = false;      // also write "<name>.bin": raw fp32 N x D (readBinEmbeddings format)
    bool text_output = true;         // the reference's text .embd (19 GB at 16 M x 128: switch off with -notext 1)
    std::string init_path;           // warm start (-init): a text .embd or, ending in ".bin", a raw fp32 N x D file, instead of randInit
    f2v_stats stats{};
    int rank = 0, world = 1;         // > 1 after join_ranks: one process per GPU, minibatch rows sharded (f2v_train_sharded)

    algorithms(CSRGraph &A_csr, std::string input, std::string outputd, INDEXTYPE dim, VALUETYPE /*gamma*/, INDEXTYPE /*bsize*/, int device = 0)
        : DIM(dim), rows(A_csr.rows), filename(input), outputdir(outputd), csr_rowptr(A_csr.rowptr), csr_colids(A_csr.colids) {
        if (f2v_create(A_csr.rowptr, A_csr.colids, A_csr.rows, A_csr.nnz, dim, device, &h) != F2V_OK) throw std::runtime_error(f2v_last_error());
    }
    ~algorithms() { f2v_destroy(h); }
    algorithms(const algorithms &) = delete;

    void srand(unsigned seed) {  // Test/Force2Vec.cpp:126
        check(f2v_srand(h, seed));
        last_seed = seed;
        seeded = true;
    }

    // options 5 / 5 -bs 1 / 6 / 6 -bs 1 / 7 (sample/algorithms.h:86-91)
    // option 1, the exact all-pairs method (sample/algorithms.cpp:344-445): symmetric init, no samples, no learning rate
    std::vector<VALUETYPE> AlgoForce2Vec(INDEXTYPE IT, INDEXTYPE TH, INDEXTYPE B) { return run(1, 0, IT, B, 0, 0.0f, "Force2Vec Parallel Wall time required:"); }
    std::vector<VALUETYPE> AlgoForce2VecNS(INDEXTYPE IT, INDEXTYPE TH, INDEXTYPE B, INDEXTYPE ns, VALUETYPE lr) { return run(5, 0, IT, B, ns, lr, "Force2Vec Parallel Wall time required:"); }
    std::vector<VALUETYPE> AlgoForce2VecNSBS(INDEXTYPE IT, INDEXTYPE TH, INDEXTYPE B, INDEXTYPE ns, VALUETYPE lr) { return run(5, 1, IT, B, ns, lr, "Force2Vec Parallel Wall time required (with BS negative samples):"); }
    std::vector<VALUETYPE> AlgoForce2VecNSRW(INDEXTYPE IT, INDEXTYPE TH, INDEXTYPE B, INDEXTYPE ns, VALUETYPE lr) { return run(6, 0, IT, B, ns, lr, "Force2Vec Parallel Wall time required:"); }
    std::vector<VALUETYPE> AlgoForce2VecNSRWBS(INDEXTYPE IT, INDEXTYPE TH, INDEXTYPE B, INDEXTYPE ns, VALUETYPE lr) { return run(6, 1, IT, B, ns, lr, "Force2Vec Parallel Wall time required (with BS negative samples):"); }
    std::vector<VALUETYPE> AlgoForce2VecNSRWEFF(INDEXTYPE IT, INDEXTYPE TH, INDEXTYPE B, INDEXTYPE ns, VALUETYPE lr) { return run(7, 0, IT, B, ns, lr, "Force2VecWNSEFF Parallel Wall time required:"); }
    // the AVX512 entry points (sample/algorithms.h:93-102): same maths on the GPU, hub rows load-balanced
    std::vector<VALUETYPE> AlgoForce2VecNS_SREAL_D128_AVXZ(INDEXTYPE IT, INDEXTYPE TH, INDEXTYPE B, INDEXTYPE ns, VALUETYPE lr) { return run(8, 0, IT, B, ns, lr, "Force2Vec Parallel Wall time required:"); }
    std::vector<VALUETYPE> AlgoForce2VecNSRW_SREAL_D128_AVXZ(INDEXTYPE IT, INDEXTYPE TH, INDEXTYPE B, INDEXTYPE ns, VALUETYPE lr) { return run(9, 0, IT, B, ns, lr, "Force2Vec Parallel Wall time required:"); }
    std::vector<VALUETYPE> AlgoForce2VecNSRWEFF_SREAL_D128_AVXZ(INDEXTYPE IT, INDEXTYPE TH, INDEXTYPE B, INDEXTYPE ns, VALUETYPE lr) { return run(10, 0, IT, B, ns, lr, "Force2VecWNSEFF Parallel Wall time required:"); }
    std::vector<VALUETYPE> AlgoForce2VecNSLB_SREAL_D128_AVXZ(INDEXTYPE IT, INDEXTYPE TH, INDEXTYPE B, INDEXTYPE ns, VALUETYPE lr) { return run(11, 0, IT, B, ns, lr, "Force2Vec Parallel Wall time required:"); }

    // Multi-GPU: this process is rank `r` of `w` (one per GPU, all constructed on the same graph, seeded alike).
    // The ranks swap the IPC handles of their matrices through files in `dir` (any directory they all see), map each
    // other (f2v_push_attach) and run the self-test together; the option methods then train sharded and only
    // rank 0 reports and writes the embedding.  No MPI, no torch: the exchange itself runs inside libf2v.
    void join_ranks(int r, int w, const std::string &dir, double timeout_s = 120.0) {
        if (w < 1 || w > F2V_PUSH_MAX_RANKS || r < 0 || r >= w) throw std::runtime_error("join_ranks: bad rank / world");
        unsigned char mine[F2V_PUSH_EXPORT_BYTES];
        check(f2v_push_export(h, mine));
        auto path = [&](int k) { return dir + "/f2v_export." + std::to_string(k); };
        {
            const std::string tmp = path(r) + ".tmp";
            FILE *f = fopen(tmp.c_str(), "wb");
            if (!f || fwrite(mine, 1, sizeof mine, f) != sizeof mine || fclose(f) != 0 || rename(tmp.c_str(), path(r).c_str()) != 0)
                throw std::runtime_error("join_ranks: cannot publish " + path(r));
        }
        std::vector<unsigned char> all((size_t)w * F2V_PUSH_EXPORT_BYTES);
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < w; k++) {
            for (;;) {
                FILE *f = fopen(path(k).c_str(), "rb");
                if (f) {
                    const size_t got = fread(all.data() + (size_t)k * F2V_PUSH_EXPORT_BYTES, 1, F2V_PUSH_EXPORT_BYTES, f);
                    fclose(f);
                    if (got == F2V_PUSH_EXPORT_BYTES) break;
                }
                if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
                    throw std::runtime_error("join_ranks: rank " + std::to_string(k) + " never published its handles in " + dir);
                std::this_thread::sleep_for(std::chrono::milliseconds(2));
            }
        }
        check(f2v_push_attach(h, (uint32_t)r, (uint32_t)w, all.data()));
        check(f2v_push_selftest(h));
        rank = r;
        world = w;
    }

    // -nearest <k>: every vertex's k nearest rows under `metric` (self excluded) as "<embd output name>.nn", one line per vertex
    // "v j1 s1 ... jk sk" (0-based ids, scores %.9g, slots past the last candidate omitted), in query blocks through the same ABI
    // as any other caller's; then the graph-reconstruction precision@k.  Call after a run (last_output names the .embd file).
    // With `lists` > 0 (-nearest-lists) the sweep goes through an index (f2v_index_*: k-means into `lists` lists, `iters` iterations
    // from `seed`; `probes` lists per query): an extra line "Index: lists <L> probes <P> candidates/query <c>", and with `check` > 0
    // (-nearest-check) the recall against the exact search over the vertices floor(i n / check), i < check.
    static constexpr uint32_t kIndexMaxLists = F2V_INDEX_MAX_LISTS, kIndexMaxProbes = F2V_INDEX_MAX_PROBES;
    std::string last_output;
    void writeNearest(uint32_t k, int metric, const char *metric_name, uint32_t lists = 0, uint32_t probes = 8, uint32_t iters = 20, uint64_t seed = 1,
                      uint32_t check_count = 0) {
        if (lists > 0) check(f2v_index_build(h, lists, iters, seed, nullptr, nullptr));
        const std::string name = last_output + ".nn";
        FILE *f = fopen(name.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + name);
        const uint32_t block = 65536;
        std::vector<uint32_t> q(block), ids((size_t)block * k);
        std::vector<float> scores((size_t)block * k);
        double seconds = 0.0, sec = 0.0;
        uint64_t hits = 0, possible = 0, candidates = 0;
        f2v_index_search_t found{};
        for (uint32_t lo = 0; lo < rows; lo += block) {
            const uint32_t cnt = rows - lo < block ? rows - lo : block;
            for (uint32_t i = 0; i < cnt; i++) q[i] = lo + i;
            const int rc = lists > 0 ? f2v_index_search_rows(h, q.data(), cnt, k, metric, F2V_NEAREST_EXCLUDE_SELF, probes, ids.data(), scores.data(), nullptr, &found)
                                     : f2v_nearest_rows(h, q.data(), cnt, k, metric, F2V_NEAREST_EXCLUDE_SELF, ids.data(), scores.data(), &sec);
            if (rc != F2V_OK) {
                fclose(f);
                throw std::runtime_error(f2v_last_error());
            }
            if (lists > 0) {
                sec = found.seconds;
                candidates += found.candidates;
            }
            seconds += sec;
            for (uint32_t i = 0; i < cnt; i++) {
                // precision@k from the ids in hand, as f2v_neighbour_recall defines it (a second sweep would only repeat the scoring)
                const uint32_t v = lo + i, *nb = csr_colids + csr_rowptr[v], deg = csr_rowptr[v + 1] - csr_rowptr[v];
                uint32_t distinct = 0;
                for (uint32_t p = 0; p < deg && distinct < k; p++)
                    if (nb[p] != v && (p == 0 || nb[p - 1] != nb[p])) distinct++;
                possible += distinct;
                for (uint32_t j = 0; j < k && ids[(size_t)i * k + j] != 0xFFFFFFFFu; j++)
                    if (std::binary_search(nb, nb + deg, ids[(size_t)i * k + j])) hits++;
                fprintf(f, "%u", lo + i);
                for (uint32_t j = 0; j < k && ids[(size_t)i * k + j] != 0xFFFFFFFFu; j++) fprintf(f, " %u %.9g", ids[(size_t)i * k + j], scores[(size_t)i * k + j]);
                fputc('\n', f);
            }
        }
        if (fclose(f) != 0) throw std::runtime_error("cannot write " + name);
        printf("Nearest: k=%u metric=%s %.6f s, precision@k %llu/%llu\n", k, metric_name, seconds, (unsigned long long)hits, (unsigned long long)possible);
        if (lists == 0) return;
        printf("Index: lists %u probes %u candidates/query %.1f\n", lists, found.nprobe, rows ? (double)candidates / rows : 0.0);
        if (check_count == 0) return;
        const uint32_t m = check_count < rows ? check_count : rows;
        std::vector<uint32_t> want((size_t)m * k);
        q.resize(m);
        ids.resize((size_t)m * k);
        for (uint32_t i = 0; i < m; i++) q[i] = (uint32_t)((uint64_t)i * rows / m);
        check(f2v_nearest_rows(h, q.data(), m, k, metric, F2V_NEAREST_EXCLUDE_SELF, want.data(), nullptr, nullptr));
        check(f2v_index_search_rows(h, q.data(), m, k, metric, F2V_NEAREST_EXCLUDE_SELF, probes, ids.data(), nullptr, nullptr, nullptr));
        uint64_t hit = 0, all = 0;
        for (uint32_t i = 0; i < m; i++)
            for (uint32_t j = 0; j < k && want[(size_t)i * k + j] != 0xFFFFFFFFu; j++) {
                all++;
                hit += std::find(ids.begin() + (size_t)i * k, ids.begin() + (size_t)(i + 1) * k, want[(size_t)i * k + j]) != ids.begin() + (size_t)(i + 1) * k ? 1 : 0;
            }
        printf("Recall@%u against the exact search (%u vertices): %.6f\n", k, m, all ? (double)hit / (double)all : 1.0);
    }

    // -cluster <k>: k-means on the trained matrix (f2v_kmeans: `restarts` seeded runs from `seed`, the one of lowest inertia) as
    // "<embd output name>.clu", one line "v label" per vertex (0-based ids), then the modularity of that labelling on the graph.
    std::vector<uint32_t> cluster_labels;  // of the last writeClusters (-separation kmeans scores them)
    void writeClusters(uint32_t k, uint32_t iters, uint32_t restarts, uint64_t seed) {
        std::vector<uint32_t> &labels = cluster_labels;
        labels.assign(rows, 0);
        f2v_kmeans_t info{};
        check(f2v_kmeans(h, k, iters, restarts, seed, nullptr, labels.data(), nullptr, nullptr, &info));
        double q = 0.0;
        check(f2v_modularity(h, labels.data(), k, &q, nullptr, nullptr, nullptr));
        const std::string name = last_output + ".clu";
        FILE *f = fopen(name.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + name);
        for (uint32_t v = 0; v < rows; v++) fprintf(f, "%u %u\n", v, labels[v]);
        if (fclose(f) != 0) throw std::runtime_error("cannot write " + name);
        printf("Clusters:%u :MODULARITY: %.17g :INERTIA: %.17g :ITERATIONS: %u :RESTART: %u\n", k, q, info.inertia, info.iterations, info.restart);
    }

    // -communities 1: the communities of the graph itself (f2v_louvain; at most `levels` levels, seeded by `seed`) as "<embd output
    // name>.com", one line "v label" per vertex (0-based ids, the format of .clu), then the reference's "Modularity: <algo> = <q>" line
    // (performancescores/runvisualization.py:152).  Beside -cluster the agreement of the k-means clusters with the communities, and
    // beside a single-label ground truth (`truth`: a labels file as -separation reads it, or empty) its agreement with them.
    // "Agreement(<what>, louvain): NMI <x> ARI <y>", or that it was skipped where the contingency table would pass the cap
    void printAgreement(const char *what, const std::vector<uint32_t> &a, uint32_t ka, const std::vector<uint32_t> &b, uint32_t kb) {
        if ((uint64_t)ka * kb > F2V_AGREEMENT_MAX_CELLS) {
            printf("Agreement(%s, louvain): skipped, %u x %u cells are more than %u\n", what, ka, kb, F2V_AGREEMENT_MAX_CELLS);
            return;
        }
        f2v_agreement_t ag{};
        check(f2v_partition_agreement(h, a.data(), ka, b.data(), kb, &ag));
        printf("Agreement(%s, louvain): NMI %.17g ARI %.17g\n", what, ag.nmi, ag.ari);
    }
    // -components 1: the connected components of the run's graph (f2v_components) as "<embd output name>.cc", one line "v label" per
    // vertex (0-based ids, the format of .com; the label is the smallest id of the component), and their counts
    void writeComponents() {
        std::vector<uint32_t> labels(rows, 0);
        f2v_components_t info{};
        check(f2v_components(h, labels.data(), nullptr, &info));
        const std::string name = last_output + ".cc";
        FILE *f = fopen(name.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + name);
        for (uint32_t v = 0; v < rows; v++) fprintf(f, "%u %u\n", v, labels[v]);
        if (fclose(f) != 0) throw std::runtime_error("cannot write " + name);
        printf("Components: %u Largest: %u Isolated: %u\n", info.components, info.largest, info.isolated);
    }
    void writeCommunities(uint32_t levels, uint64_t seed, const std::string &truth) {
        std::vector<uint32_t> labels(rows, 0);
        f2v_louvain_t info{};
        check(f2v_louvain(h, seed, levels, 64, labels.data(), nullptr, nullptr, &info));
        const std::string name = last_output + ".com";
        FILE *f = fopen(name.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + name);
        for (uint32_t v = 0; v < rows; v++) fprintf(f, "%u %u\n", v, labels[v]);
        if (fclose(f) != 0) throw std::runtime_error("cannot write " + name);
        printf("Modularity: Louvain = %.17g Communities: %u Levels: %u\n", info.modularity, info.communities, info.levels);
        const uint32_t K = std::max(info.communities, 1u);
        if (!cluster_labels.empty()) {
            uint32_t k = 0;
            for (uint32_t l : cluster_labels) k = std::max(k, l + 1);
            printAgreement("kmeans", cluster_labels, k, labels, K);
        }
        if (!truth.empty()) {
            std::vector<bool> seen;
            const std::vector<std::vector<uint32_t>> all = readLabels(truth, F2V_SEPARATION_MAX_CLUSTERS, "-communities", seen);
            std::vector<uint32_t> given(rows, F2V_LABEL_NONE);
            uint32_t k = 1;
            for (uint32_t v = 0; v < rows; v++)
                if (!all[v].empty()) {
                    given[v] = all[v][0];
                    k = std::max(k, given[v] + 1);
                }
            printAgreement("labels", given, k, labels, K);
        }
    }

    // -classify <labels file>: node classification as the reference scores it (performancescores/runnodeclassclust.py).  The file holds
    // lines "vertex label" with 1-based vertex ids; a vertex may have several lines; labels are 0 .. C - 1, C <= 64.  For split
    // s = 0 .. splits - 1 the labelled vertices are ordered by key(v) = mix64(mix64(seed + s) ^ v) ascending (mix64: the splitmix64
    // finaliser of include/f2v.h), ties by id; the first int(L * frac) of the L train f2v_logreg_fit (lambda 1, tol 1e-4, 100
    // iterations), every other one is predicted as many labels as it has: its largest decision values, ties to the lower class.
    // Prints the means of the splits' micro and macro F1 in percent.
    static uint64_t mix64(uint64_t z) {
        z += 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    // The labels reader of -classify and -separation: lines "vertex label", 1-based vertex ids, labels 0 .. max_labels - 1; a vertex
    // may have several lines.  -> the labels of every vertex in file order; seen[l]: label l occurs.
    std::vector<std::vector<uint32_t>> readLabels(const std::string &path, long max_labels, const char *flag, std::vector<bool> &seen) {
        FILE *f = fopen(path.c_str(), "r");
        if (!f) throw std::runtime_error("cannot read " + path);
        std::vector<std::vector<uint32_t>> labels(rows);
        long v = 0, l = 0;
        while (fscanf(f, "%ld %ld", &v, &l) == 2) {
            if (v < 1 || v > (long)rows || l < 0 || l >= max_labels) {
                fclose(f);
                throw std::runtime_error(std::string(flag) + ": \"" + std::to_string(v) + " " + std::to_string(l) + "\" is outside the graph's vertices or the " +
                                         std::to_string(max_labels) + " classes");
            }
            labels[v - 1].push_back((uint32_t)l);
            if (seen.size() <= (size_t)l) seen.resize(l + 1, false);
            seen[l] = true;
        }
        fclose(f);
        return labels;
    }
    void classify(const std::string &path, double frac, uint32_t splits, uint64_t seed) {
        std::vector<bool> seen;
        const std::vector<std::vector<uint32_t>> labels = readLabels(path, F2V_LOGREG_MAX_CLASSES, "-classify", seen);
        const uint32_t C = (uint32_t)seen.size();
        if (C == 0 || std::find(seen.begin(), seen.end(), false) != seen.end()) throw std::runtime_error("-classify: the labels must be 0 .. C - 1, each used");
        std::vector<uint32_t> labelled;
        for (uint32_t u = 0; u < rows; u++)
            if (!labels[u].empty()) labelled.push_back(u);
        const size_t L = labelled.size(), cv = (size_t)((double)L * frac);
        if (cv == 0 || cv == L) throw std::runtime_error("-classify: the split leaves no training or no test vertex");
        const uint32_t P = DIM + 1;
        double micro_sum = 0.0, macro_sum = 0.0;
        for (uint32_t s = 0; s < splits; s++) {
            const uint64_t sm = mix64(seed + s);
            std::vector<std::pair<uint64_t, uint32_t>> keyed(L);
            for (size_t i = 0; i < L; i++) keyed[i] = {mix64(sm ^ (uint64_t)labelled[i]), labelled[i]};
            std::sort(keyed.begin(), keyed.end());
            std::vector<uint32_t> ids(L);
            for (size_t i = 0; i < L; i++) ids[i] = keyed[i].second;
            std::vector<uint8_t> y(L * C, 0);
            for (size_t i = 0; i < L; i++)
                for (uint32_t c : labels[ids[i]]) y[i * C + c] = 1;
            std::vector<double> W((size_t)C * P), z((L - cv) * C);
            std::vector<f2v_logreg_t> info(C);
            check(f2v_logreg_fit(h, ids.data(), nullptr, (uint32_t)cv, F2V_PAIR_HADAMARD, y.data(), C, 1.0, 1e-4, 100, W.data(), info.data()));
            check(f2v_logreg_decision(h, ids.data() + cv, nullptr, (uint32_t)(L - cv), F2V_PAIR_HADAMARD, W.data(), C, z.data(), nullptr));
            std::vector<double> tp(C, 0.0), fp(C, 0.0), fn(C, 0.0);
            std::vector<uint32_t> order(C);
            for (size_t i = cv; i < L; i++) {
                const double *zi = z.data() + (i - cv) * C;
                const uint8_t *yi = y.data() + i * C;
                uint32_t k = 0;
                for (uint32_t c = 0; c < C; c++) {
                    order[c] = c;
                    k += yi[c];
                }
                std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return zi[a] > zi[b]; });
                std::vector<uint8_t> pred(C, 0);
                for (uint32_t j = 0; j < k; j++) pred[order[j]] = 1;
                for (uint32_t c = 0; c < C; c++) {
                    tp[c] += yi[c] && pred[c];
                    fp[c] += !yi[c] && pred[c];
                    fn[c] += yi[c] && !pred[c];
                }
            }
            double tps = 0.0, fps = 0.0, fns = 0.0, per = 0.0;
            for (uint32_t c = 0; c < C; c++) {
                tps += tp[c];
                fps += fp[c];
                fns += fn[c];
                const double den = 2 * tp[c] + fp[c] + fn[c];
                per += den > 0 ? 2 * tp[c] / den : 0.0;
            }
            const double den = 2 * tps + fps + fns;
            micro_sum += 100.0 * (den > 0 ? 2 * tps / den : 0.0);
            macro_sum += 100.0 * (per / C);
        }
        printf("Classify: frac %g :F1-MICRO: %.17g :F1-MACRO: %.17g\n", frac, micro_sum / splits, macro_sum / splits);
    }

    // -separation <labels file | kmeans>: the silhouette and the Davies-Bouldin score of a labelling in the embedding space, the line
    // performancescores/runvisualization.py prints.  A labels file is read as -classify reads it (a vertex's first label counts,
    // labels 0 .. 1023); a vertex the file does not name takes no part (F2V_LABEL_NONE).  "kmeans": the labels of this run's -cluster.
    // sample > 0: the silhouette of that many labelled vertices, the first of the order key(v) = mix64(mix64(seed) ^ v) ascending,
    // ties by id (as f2v_kmeans seeds its rows), each scored against all labelled vertices; 0: of every labelled vertex.
    void separation(const std::string &what, uint32_t sample, uint64_t seed) {
        std::vector<uint32_t> labels;
        if (what == "kmeans") {
            labels = cluster_labels;
        } else {
            std::vector<bool> seen;
            const std::vector<std::vector<uint32_t>> all = readLabels(what, F2V_SEPARATION_MAX_CLUSTERS, "-separation", seen);
            labels.assign(rows, F2V_LABEL_NONE);
            for (uint32_t v = 0; v < rows; v++)
                if (!all[v].empty()) labels[v] = all[v][0];
        }
        uint32_t k = 0;
        std::vector<std::pair<uint64_t, uint32_t>> keyed;
        const uint64_t sm = mix64(seed);
        for (uint32_t v = 0; v < rows; v++) {
            if (labels[v] == F2V_LABEL_NONE) continue;
            k = std::max(k, labels[v] + 1);
            if (sample) keyed.push_back({mix64(sm ^ (uint64_t)v), v});
        }
        std::vector<uint32_t> ids;
        if (sample) {
            std::sort(keyed.begin(), keyed.end());
            for (size_t i = 0; i < keyed.size() && i < sample; i++) ids.push_back(keyed[i].second);
        }
        double sil = 0.0, db = 0.0;
        check(f2v_silhouette(h, labels.data(), k, sample ? ids.data() : nullptr, (uint32_t)ids.size(), nullptr, nullptr, &sil, nullptr));
        check(f2v_davies_bouldin(h, labels.data(), k, &db, nullptr, nullptr, nullptr, nullptr));
        printf("silhouette: %.17g davies_bouldin: %.17g\n", sil, db);
    }

    // -layout <d>: the projection of the trained matrix onto its first d principal components (f2v_pca) as "<embd output name>.lay",
    // one line "v y1 ... yd" per vertex (1-based ids, %g as the .embd writer), then the line performancescores/runvisualization.py
    // prints for its picture, extended by the mirror score: f2v_trustworthiness of the layout with k neighbours.  sample > 0: over
    // that many vertices, the first of the order key(v) = mix64(mix64(seed) ^ v) ascending, ties by id (as -separation-sample), each
    // ranked against all vertices; 0: over every vertex.
    // tsne (-layout-method tsne): the coordinates are f2v_tsne's over every vertex (d = 2 or 3) with the PCA start, and the second
    // line reports the run instead of the explained variance.
    void layout(uint32_t d, uint32_t k, uint32_t sample, uint64_t seed, bool tsne = false, double perplexity = 30.0, uint32_t iters = 1000) {
        std::vector<float> y((size_t)rows * d);
        std::vector<double> var(d);
        f2v_pca_t info{};
        f2v_tsne_t run{};
        if (tsne) {
            f2v_tsne_params par{};
            par.perplexity = perplexity;
            par.iters = iters;
            check(f2v_tsne(h, nullptr, rows, d, &par, nullptr, nullptr, nullptr, nullptr, y.data(), &run));
        } else {
            check(f2v_pca(h, d, y.data(), nullptr, nullptr, var.data(), &info));
        }
        const std::string name = last_output + ".lay";
        FILE *f = fopen(name.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + name);
        for (uint32_t v = 0; v < rows; v++) {
            fprintf(f, "%u", v + 1);
            for (uint32_t c = 0; c < d; c++) fprintf(f, " %g", y[(size_t)v * d + c]);
            fputc('\n', f);
        }
        if (fclose(f) != 0) throw std::runtime_error("cannot write " + name);
        std::vector<uint32_t> ids;
        if (sample) {
            std::vector<std::pair<uint64_t, uint32_t>> keyed;
            const uint64_t sm = mix64(seed);
            for (uint32_t v = 0; v < rows; v++) keyed.push_back({mix64(sm ^ (uint64_t)v), v});
            std::sort(keyed.begin(), keyed.end());
            for (size_t i = 0; i < keyed.size() && i < sample; i++) ids.push_back(keyed[i].second);
        }
        f2v_trust_t t{};
        check(f2v_trustworthiness(h, y.data(), d, k, sample ? ids.data() : nullptr, (uint32_t)ids.size(), nullptr, nullptr, &t));
        double kept = 0.0;
        for (uint32_t c = 0; c < d; c++) kept += var[c];
        printf("TrustWorthiness: %.17g Continuity: %.17g\n", t.trustworthiness, t.continuity);
        if (tsne) {
            printf("Layout: d=%u neighbours=%u samples=%u :METHOD: tsne :PERPLEXITY: %g :ITERATIONS: %u :KL: %.17g :OVERLAP: %.17g\n", d, k,
                   sample ? (uint32_t)ids.size() : rows, perplexity, iters, run.kl, t.overlap);
            return;
        }
        printf("Layout: d=%u neighbours=%u samples=%u :EXPLAINED-VARIANCE: %.17g :OVERLAP: %.17g :SWEEPS: %u\n", d, k, sample ? (uint32_t)ids.size() : rows,
               info.total_variance > 0 ? kept / info.total_variance : 0.0, t.overlap, info.sweeps);
    }

    // -foldin <file>: vectors for vertices that were not in the graph (f2v_fold_in).  Each line of the file is "<name> <nbr> <nbr> ..."
    // with 1-based ids of existing vertices, in summation order; the output "<embd output name>.fold" is .embd text -- "<m> <D>", then
    // per line the name and the vector's values with %g and a trailing space.  The negative samples are seeded by -seed.
    void foldIn(const std::string &path, int option, uint32_t iters, INDEXTYPE ns, VALUETYPE lr, int init_kind, uint64_t seed) {
        std::ifstream in(path);
        if (!in) throw std::runtime_error("-foldin: cannot read " + path);
        std::vector<std::string> names;
        std::vector<uint32_t> rowptr{0}, colids;
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream fields(line);
            std::string name;
            if (!(fields >> name)) continue;
            long long id;
            while (fields >> id) {
                if (id < 1 || id > (long long)rows) throw std::runtime_error("-foldin: " + name + " names vertex " + std::to_string(id) + " of " + std::to_string(rows));
                colids.push_back((uint32_t)(id - 1));
            }
            if (!fields.eof()) throw std::runtime_error("-foldin: the line of " + name + " holds something that is not a vertex id");
            names.push_back(name);
            rowptr.push_back((uint32_t)colids.size());
        }
        const uint32_t m = (uint32_t)names.size();
        std::vector<float> y((size_t)m * DIM);
        f2v_fold_t info{};
        colids.push_back(0);  // (an address where every list is empty)
        check(f2v_fold_in(h, option, rowptr.data(), colids.data(), m, iters, ns, lr, init_kind, nullptr, seed, 0, y.data(), &info));
        const std::string name = last_output + ".fold";
        FILE *f = fopen(name.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + name);
        fprintf(f, "%u %u\n", m, (unsigned)DIM);
        for (uint32_t q = 0; q < m; q++) {
            fprintf(f, "%s ", names[q].c_str());
            for (uint32_t d = 0; d < DIM; d++) fprintf(f, "%g ", (double)y[(size_t)q * DIM + d]);
            fputc('\n', f);
        }
        if (fclose(f) != 0) throw std::runtime_error("cannot write " + name);
        printf("Fold-in: %u vertices, %u iterations, %llu interactions in %.6f s on the GPU -> %s\n", m, iters, (unsigned long long)info.pairs, info.seconds, name.c_str());
    }

    // -linkpredict <feature>: link prediction as the reference scores it (performancescores/runlinkpredict.py).  The pair set is
    // f2v_link_pairs(ratio, seed): every edge once, `ratio` times as many non-neighbours per vertex, shuffled; f2v_logreg_fit (lambda 1,
    // tol 1e-4, 100 iterations) on the first int(M * frac) pairs with the feature, z > 0 predicts an edge for the others.  Prints the
    // reference's line -- accuracy and the macro and micro F1 over the labels that occur among the predictions, as fractions of 1 --
    // and returns the three in percent, computed as Engine.link_predict computes them.
    struct LinkScores {
        double accuracy, f1_macro, f1_micro;
    };
    LinkScores linkPredict(int feature, double frac, uint32_t ratio, uint64_t seed) {
        static const char *const names[] = {"Hadamard", "L1", "L2", "Average"};
        uint64_t M = 0;
        check(f2v_link_pairs(h, ratio, seed, nullptr, nullptr, nullptr, 0, &M, nullptr));
        if (M > 0xFFFFFFFFull) throw std::runtime_error("-linkpredict: more than 2^32 - 1 pairs");
        const size_t cv = (size_t)((double)M * frac);
        if (cv == 0 || cv == M) throw std::runtime_error("-linkpredict: the split leaves no training or no test pair");
        std::vector<uint32_t> u(M), v(M);
        std::vector<uint8_t> y(M);
        check(f2v_link_pairs(h, ratio, seed, u.data(), v.data(), y.data(), M, &M, nullptr));
        const size_t tests = M - cv;
        std::vector<double> W((size_t)DIM + 1), z(tests);
        f2v_logreg_t info{};
        check(f2v_logreg_fit(h, u.data(), v.data(), (uint32_t)cv, feature, y.data(), 1, 1.0, 1e-4, 100, W.data(), &info));
        check(f2v_logreg_decision(h, u.data() + cv, v.data() + cv, (uint32_t)tests, feature, W.data(), 1, z.data(), nullptr));
        double tp[2] = {0, 0}, fp[2] = {0, 0}, fn[2] = {0, 0}, hits = 0;
        for (size_t i = 0; i < tests; i++) {
            const int pred = z[i] > 0, truth = y[cv + i] != 0;
            hits += pred == truth;
            for (int c = 0; c < 2; c++) {
                tp[c] += truth == c && pred == c;
                fp[c] += truth != c && pred == c;
                fn[c] += truth == c && pred != c;
            }
        }
        double tps = 0.0, fps = 0.0, fns = 0.0, per = 0.0, classes = 0.0;
        for (int c = 0; c < 2; c++) {
            if (tp[c] + fp[c] == 0) continue;  // the label does not occur among the predictions
            classes += 1;
            tps += tp[c];
            fps += fp[c];
            fns += fn[c];
            const double den = 2 * tp[c] + fp[c] + fn[c];
            per += den > 0 ? 2 * tp[c] / den : 0.0;
        }
        const double den = 2 * tps + fps + fns;
        const LinkScores s{100.0 * (hits / (double)tests), 100.0 * (per / classes), 100.0 * (den > 0 ? 2 * tps / den : 0.0)};
        printf("Link predictions(%s): %g :Accuracy: %.17g F1-macro: %.17g F1-micro: %.17g\n", names[feature], frac, s.accuracy / 100.0, s.f1_macro / 100.0, s.f1_micro / 100.0);
        return s;
    }

    // -holdout <f>: held-out link prediction of the embedding this object trained on `split.train`.  Writes "<embd output name>.held",
    // one line "u v y" per pair (1-based ids; the hidden edges, y = 1, then the non-edges, y = 0), ranks the pairs by the embedding's
    // own similarity (f2v_pair_scores, f2v_ranking) and prints "Held-out link prediction(<metric>): <H> edges :AUC: <a> AP: <p>"; with
    // `feature` >= 0 also by the decision values of a logistic regression fitted on every pair of f2v_link_pairs(ratio, seed) of the
    // training graph, under the feature's name.  Computed as Engine.heldout_scores computes them.
    struct HeldScores {
        double auc, ap, classifier_auc, classifier_ap;
    };
    HeldScores heldOut(const Holdout &split, int metric, const char *metric_name, int feature, uint32_t ratio, uint64_t seed) {
        static const char *const names[] = {"Hadamard", "L1", "L2", "Average"};
        const size_t H = split.held_u.size(), m = H + split.neg_u.size();
        std::vector<uint32_t> u(split.held_u), v(split.held_v);
        u.insert(u.end(), split.neg_u.begin(), split.neg_u.end());
        v.insert(v.end(), split.neg_v.begin(), split.neg_v.end());
        std::vector<uint8_t> y(m, 0);
        std::fill(y.begin(), y.begin() + H, (uint8_t)1);
        const std::string name = last_output + ".held";
        FILE *f = fopen(name.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + name);
        for (size_t i = 0; i < m; i++) fprintf(f, "%u %u %u\n", u[i] + 1, v[i] + 1, (unsigned)y[i]);
        if (fclose(f) != 0) throw std::runtime_error("cannot write " + name);
        std::vector<float> s(m);
        std::vector<double> z(m);
        check(f2v_pair_scores(h, u.data(), v.data(), m, metric, s.data(), nullptr));
        for (size_t i = 0; i < m; i++) z[i] = (double)s[i];
        f2v_ranking_t own{}, clf{};
        check(f2v_ranking(h, z.data(), y.data(), m, &own));
        printf("Held-out link prediction(%s): %zu edges :AUC: %.17g AP: %.17g\n", metric_name, H, own.auc, own.ap);
        if (feature >= 0) {
            uint64_t M = 0;
            check(f2v_link_pairs(h, ratio, seed, nullptr, nullptr, nullptr, 0, &M, nullptr));
            if (M == 0 || M > 0xFFFFFFFFull || m > 0xFFFFFFFFull) throw std::runtime_error("-holdout with -linkpredict: no pair of the training graph to fit on, or more than 2^32 - 1");
            std::vector<uint32_t> tu(M), tv(M);
            std::vector<uint8_t> ty(M);
            check(f2v_link_pairs(h, ratio, seed, tu.data(), tv.data(), ty.data(), M, &M, nullptr));
            std::vector<double> W((size_t)DIM + 1);
            f2v_logreg_t info{};
            check(f2v_logreg_fit(h, tu.data(), tv.data(), (uint32_t)M, feature, ty.data(), 1, 1.0, 1e-4, 100, W.data(), &info));
            check(f2v_logreg_decision(h, u.data(), v.data(), (uint32_t)m, feature, W.data(), 1, z.data(), nullptr));
            check(f2v_ranking(h, z.data(), y.data(), m, &clf));
            printf("Held-out link prediction(%s): %zu edges :AUC: %.17g AP: %.17g\n", names[feature], H, clf.auc, clf.ap);
        }
        return HeldScores{own.auc, own.ap, clf.auc, clf.ap};
    }

    // -holdout-baselines 1: the yardstick of heldOut.  The neighbourhood scores of the same pairs on the training graph (this object's
    // handle: f2v_pair_neighbourhood), each kind ranked by f2v_ranking; prints, in kind order, "Held-out baseline(<cn|jaccard|aa|ra|pa>):
    // <H> edges :AUC: <a> AP: <p>".  Computed as Engine.heldout_baselines computes them.
    void heldOutBaselines(const Holdout &split) {
        static const char *const names[] = {"cn", "jaccard", "aa", "ra", "pa"};
        const size_t H = split.held_u.size(), m = H + split.neg_u.size();
        std::vector<uint32_t> u(split.held_u), v(split.held_v);
        u.insert(u.end(), split.neg_u.begin(), split.neg_u.end());
        v.insert(v.end(), split.neg_v.begin(), split.neg_v.end());
        std::vector<uint8_t> y(m, 0);
        std::fill(y.begin(), y.begin() + H, (uint8_t)1);
        std::vector<double> s(5 * m);
        check(f2v_pair_neighbourhood(h, u.data(), v.data(), m, F2V_NB_ALL, s.data(), nullptr));
        for (size_t k = 0; k < 5; k++) {
            f2v_ranking_t r{};
            check(f2v_ranking(h, s.data() + k * m, y.data(), m, &r));
            printf("Held-out baseline(%s): %zu edges :AUC: %.17g AP: %.17g\n", names[k], H, r.auc, r.ap);
        }
    }

    // -holdout-ranks <s>: the filtered rank of the hidden edges among all vertices (this object's handle, the training graph's:
    // f2v_pair_ranks with both exclusions).  sample < 0: every hidden edge; 0 < sample < H: those of index floor(j H / sample).  Each
    // edge {a, b} gives the pairs (a, b) and (b, a).  Writes "<embd output name>.rank", one line "u v greater equal" per pair (1-based
    // ids), and prints "Held-out ranks(<metric>): <P> pairs :MRR: <m> MeanRank: <r> Hits@1: <a> Hits@10: <b> Hits@50: <c> Hits@100: <d>",
    // the hits as fractions of P.  Computed as Engine.heldout_ranks computes them.
    void heldOutRanks(const Holdout &split, int metric, const char *metric_name, long sample) {
        const uint64_t H = split.held_u.size(), take = sample > 0 && (uint64_t)sample < H ? (uint64_t)sample : H;
        std::vector<uint32_t> u, v;
        u.reserve(2 * take);
        v.reserve(2 * take);
        for (uint64_t j = 0; j < take; j++) {
            const uint64_t e = take == H ? j : (uint64_t)(((unsigned __int128)j * H) / take);
            u.push_back(split.held_u[e]);
            v.push_back(split.held_v[e]);
            u.push_back(split.held_v[e]);
            v.push_back(split.held_u[e]);
        }
        const uint64_t P = u.size();
        static const uint32_t ks[4] = {1, 10, 50, 100};
        std::vector<uint32_t> greater(P), equal(P);
        uint64_t hits[4] = {0, 0, 0, 0};
        f2v_pair_ranks_t info{};
        check(f2v_pair_ranks(h, u.data(), v.data(), P, metric, F2V_NEAREST_EXCLUDE_SELF | F2V_NEAREST_EXCLUDE_NEIGHBOURS, greater.data(), equal.data(), ks, 4, hits, &info));
        const std::string name = last_output + ".rank";
        FILE *f = fopen(name.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + name);
        for (uint64_t i = 0; i < P; i++) fprintf(f, "%u %u %u %u\n", u[i] + 1, v[i] + 1, greater[i], equal[i]);
        if (fclose(f) != 0) throw std::runtime_error("cannot write " + name);
        const double p = P ? (double)P : 1.0;
        printf("Held-out ranks(%s): %llu pairs :MRR: %.17g MeanRank: %.17g Hits@1: %.17g Hits@10: %.17g Hits@50: %.17g Hits@100: %.17g\n", metric_name,
               (unsigned long long)P, P ? info.mrr : 0.0, P ? info.mean_rank : 0.0, hits[0] / p, hits[1] / p, hits[2] / p, hits[3] / p);
    }

    // writeToFile, sample/algorithms.h:118-136 (file name rule in f2v_output_name)
    void writeToFile(int option, int bs, INDEXTYPE B, INDEXTYPE IT, INDEXTYPE ns) {
        char name[4096];
        check(f2v_output_name(filename.c_str(), outputdir.c_str(), option, bs, B, DIM, IT, ns, name, sizeof name));
        std::cout << "Creating output file in following directory:" << name << std::endl;
        last_output = name;
        std::vector<float> x((size_t)rows * DIM);
        check(f2v_get_embeddings(h, x.data()));
        if (text_output) check(f2v_write_embd(name, x.data(), rows, DIM));
        if (binary_output) check(f2v_write_embd_bin((std::string(name) + ".bin").c_str(), x.data(), rows, DIM));
    }

   private:
    const INDEXTYPE *csr_rowptr, *csr_colids;  // the caller's graph (it outlives this object): writeNearest counts hits in it
    unsigned last_seed = 1;
    bool seeded = false;  // srand() was the last thing to touch the handle's rand() stream: a lost run can be repeated from it
    static void check(int rc) {
        if (rc != F2V_OK) throw std::runtime_error(f2v_last_error());
    }
    int64_t param(const char *name) {
        int64_t v = 0;
        check(f2v_get_param(h, name, &v));
        return v;
    }
    // randInitF / randInit (algorithms.cpp:38-53) -- or the embedding file of a warm start
    void init(int math) {
        if (init_path.empty()) {
            check(f2v_init_embeddings(h, math == 5 ? F2V_INIT_SYMMETRIC : F2V_INIT_UNIT));
            return;
        }
        const std::string ext = ".bin";
        if (init_path.size() > ext.size() && init_path.compare(init_path.size() - ext.size(), ext.size(), ext) == 0) {
            std::vector<float> x((size_t)rows * DIM);
            check(f2v_read_embd_bin(init_path.c_str(), rows, DIM, x.data()));
            check(f2v_set_embeddings(h, x.data()));
        } else {
            uint32_t n = 0, d = 0;
            float *x = nullptr;
            check(f2v_read_embd(init_path.c_str(), &n, &d, &x));
            const bool fits = n == rows && d == DIM;
            if (fits) check(f2v_set_embeddings(h, x));
            f2v_free(x);
            if (!fits) throw std::runtime_error("-init: " + init_path + " holds " + std::to_string(n) + " x " + std::to_string(d) + " values, the run needs " +
                                                std::to_string(rows) + " x " + std::to_string(DIM));
        }
    }
    std::vector<VALUETYPE> run(int option, int bs, INDEXTYPE IT, INDEXTYPE B, INDEXTYPE ns, VALUETYPE lr, const char *msg) {
        // the reference's timer spans randInit + the epoch loop (algorithms.cpp:557-558, 647)
        auto t0 = std::chrono::steady_clock::now();
        const int math = (option == 1 || option == 5 || option == 8 || option == 11) ? 5 : 6;
        init(math);
        if (world > 1) {
            check(f2v_train_sharded(h, option, IT, B, ns, lr, bs, &gpu_train_seconds));
        } else {
            // A launch whose in-grid waits gave up (another tenant of the GPU kept its workgroups from starting) is not the end
            // of the run: f2v_train repeats the call by itself from its snapshot ("recover"); where it could not (no room for
            // the snapshot, "recover" = 0) the handle has already switched to launches without in-grid waits, and the run is
            // repeated here from its seed -- same process, same bytes as a healthy run.
            const int64_t before = param("recoveries");
            const bool waits_before = param("merge_finalize") != 0;
            const bool repeatable = seeded;
            seeded = false;
            int rc = f2v_train(h, option, IT, B, ns, lr, bs, &gpu_train_seconds);
            // (a lost launch is the one failure that switches "merge_finalize" from 1 to 0; any other F2V_ESTATE -- and a handle
            // whose in-grid waits the caller had switched off -- is reported, not retried)
            if (rc == F2V_ESTATE && repeatable && waits_before && param("merge_finalize") == 0) {
                std::cerr << "Force2Vec: " << f2v_last_error() << "\nForce2Vec: running again from seed " << last_seed << std::endl;
                check(f2v_srand(h, last_seed));
                init(math);
                rc = f2v_train(h, option, IT, B, ns, lr, bs, &gpu_train_seconds);
            } else if (rc == F2V_OK && param("recoveries") != before) {
                std::cerr << "Force2Vec: " << f2v_last_error() << std::endl;
            }
            check(rc);
        }
        auto t1 = std::chrono::steady_clock::now();
        const double sec = std::chrono::duration<double>(t1 - t0).count();
        f2v_get_stats(h, &stats);
        if (rank == 0) {  // every replica is complete; one of them reports
            std::cout << msg << sec << " seconds" << std::endl;
            writeToFile(option, bs, B, IT, ns);
        }
        return std::vector<VALUETYPE>{(VALUETYPE)sec};
    }
};

}  // namespace f2v_host
#endif
