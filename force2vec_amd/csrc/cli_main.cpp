// cli_main.cpp -- ./bin/Force2Vec: the reference's process boundary (Test/Force2Vec.cpp:49-199) over libf2v.
// Same flags, defaults, exit codes, output file names and Results.txt line, so shell scripts and the
// reference's Python scorers keep working; the parsing itself is table driven.  `-threads` and `-gamma` are
// accepted and unused (the force kernels run on the MI355X).
// Extra flags: -device <int>, -seed <int> (default 1 = the reference's srand(1)), -cache 1 (keep / reuse a
// binary CSR "<input>.f2vcsr"), -binout 1 (also write "<output>.embd.bin", raw fp32 N x D), -notext 1, -fastrng 1
// (NON-parity fast mode: device-side initial embeddings and option-7 walks), -gpus <n> (one forked process per GPU,
// devices -device .. -device+n-1: every minibatch's rows sharded over them, new rows pushed over xGMI --
// f2v_train_sharded; the ranks meet through files in a private temporary directory; same output, written by rank 0),
// -loss <k> (print the training objective after every k-th epoch and the last, in the line the reference has commented out),
// -nearest <k> [-metric dot|l2|cos] (after training: every vertex's k nearest rows as "<embd output name>.nn" and the
// graph-reconstruction precision@k; default metric: the option's own similarity; with -nearest-lists <L> [-nearest-probes <p>]
// [-nearest-iters <i>] [-nearest-check <s>] through an inverted-file index: L k-means lists, p of them scored per query), -cluster <k> [-cluster-iters <n>]
// [-cluster-restarts <r>] (after training: k-means on the embedding as "<embd output name>.clu" and its modularity on the graph),
// -classify <labels file> [-classify-frac <f>] [-classify-splits <s>] (after training: node-classification F1 of the embedding),
// -separation <labels file | kmeans> [-separation-sample <n>] (after training: the labelling's silhouette and Davies-Bouldin score),
// -layout <d> [-layout-method pca|tsne] [-layout-perplexity <p>] [-layout-iters <n>] [-layout-neighbours <k>] [-layout-sample <n>] (after training: the d-dimensional principal-component -- or exact t-SNE -- layout as
// "<embd output name>.lay" and its trustworthiness and continuity), -foldin <file> [-foldin-iters <n>] [-foldin-init mean|random] (after
// training, or on -init <file> with -iter 0: vectors for new vertices, one "<name> <nbr> <nbr> ..." line each, as "<embd output name>.fold"),
// -linkpredict <hadamard|l1|l2|average> [-linkpredict-frac <f>] [-linkpredict-ratio <r>] (after training, or on -init <file> with -iter 0:
// the reference's link-prediction scores of the embedding on the pair set f2v_link_pairs builds from the graph),
// -communities 1 [-communities-levels <L>] [-communities-seed <s>] (after training, or on -init <file> with -iter 0: the communities of the
// graph itself as "<embd output name>.com", their modularity, and their agreement with the -cluster clusters and the ground truth),
// -components 1 (the connected components of the run's graph as "<embd output name>.cc" and their counts; needs no training),
// -holdout <f> [-holdout-ratio <r>] [-holdout-metric dot|l2|cos] [-holdout-keep anchor|forest] (held-out link prediction: a share of the edges is hidden BEFORE training,
// the run trains on the rest -- the .embd is then the training graph's embedding -- and the hidden edges are ranked against non-edges:
// "<embd output name>.held" and ROC-AUC / average precision; with -linkpredict also by the classifier's decision values; with
// -holdout-baselines 1 also by the five neighbourhood scores of the training graph, the yardstick; with -holdout-ranks <s> every hidden
// edge -- or s of them -- is also placed among ALL vertices: "<embd output name>.rank", MRR, mean rank and Hits@K).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <thread>

#include <sys/wait.h>
#include <unistd.h>

#include "algorithms.hpp"

using namespace f2v_host;

namespace {

struct Settings {
    std::string input, output, init;
    long batch = 384, iter = 1200, threads = (long)std::thread::hardware_concurrency(), dim = 128, nsamples = 5, option = 5, bs = 0;
    long device = 0, seed = 1, cache = 0, binout = 0, fastrng = 0, notext = 0, gpus = 1, samegpu = 0, loss = 0, nearest = 0, cluster = 0, cluster_iters = 300, cluster_restarts = 10;
    std::string metric, classify, separation, foldin, foldin_init = "mean", layout_method = "pca";
    long nearest_lists = 0, nearest_probes = 0, nearest_iters = 20, nearest_check = 0;  // nearest_probes 0: not given (8)
    long layout_iters = 1000;
    double layout_perplexity = 30.0;
    long foldin_iters = 300;
    std::string linkpredict;
    long communities = 0, communities_levels = 32, communities_seed = 1;
    long components = 0;
    std::string holdout_keep;
    long linkpredict_ratio = 2;
    double linkpredict_frac = 0.5;
    double holdout = -1.0;  // not given
    long holdout_ratio = 1;
    long holdout_baselines = 0;
    long holdout_ranks = 0;
    std::string holdout_metric;
    long classify_splits = 10, separation_sample = 0, layout = 0, layout_neighbours = 5, layout_sample = 0;
    double gamma = 1.0, lr = 0.02, classify_frac = 0.1;
};

enum class Kind { Text, Integer, Real };
struct Flag {
    const char *name;
    Kind kind;
    void *target;
    const char *help;
};

// option number -> the name the reference prints and logs (Test/Force2Vec.cpp:80-102) and the method that runs it
struct Variant {
    int option;
    const char *name;
    std::vector<VALUETYPE> (algorithms::*plain)(INDEXTYPE, INDEXTYPE, INDEXTYPE, INDEXTYPE, VALUETYPE);
    std::vector<VALUETYPE> (algorithms::*with_bs)(INDEXTYPE, INDEXTYPE, INDEXTYPE, INDEXTYPE, VALUETYPE);
};
const Variant kVariants[] = {
    {1, "Force2Vec(n^2)", nullptr, nullptr},  // AlgoForce2Vec(ITERATIONS, NUMOFTHREADS, BATCHSIZE): no samples, no learning rate
    {5, "Force2Vec:t-distribution with negative sampling", &algorithms::AlgoForce2VecNS, &algorithms::AlgoForce2VecNSBS},
    {6, "Force2Vec:sigmoid with negative sampling", &algorithms::AlgoForce2VecNSRW, &algorithms::AlgoForce2VecNSRWBS},
    {7, "Force2Vec:sigmoid based random-walk", &algorithms::AlgoForce2VecNSRWEFF, nullptr},
    {8, "Force2Vec:AVX512 support for t-distribution with negative sampling", &algorithms::AlgoForce2VecNS_SREAL_D128_AVXZ, nullptr},
    {9, "Force2Vec:AVX512 support for sigmoid with negative sampling", &algorithms::AlgoForce2VecNSRW_SREAL_D128_AVXZ, nullptr},
    {10, "Force2Vec:AVX512 support for sigmoid based random-walk", &algorithms::AlgoForce2VecNSRWEFF_SREAL_D128_AVXZ, nullptr},
    {11, "Force2Vec:Load-balancing with AVX512 support for t-distribution with negative sampling", &algorithms::AlgoForce2VecNSLB_SREAL_D128_AVXZ, nullptr},
};

void usage(const Flag *flags, size_t count) {
    printf("\nUsage of Force2Vec tool:\n");
    for (size_t k = 0; k < count; k++) printf("%s %s\n", flags[k].name, flags[k].help);
    printf("-h, show help message.\n");
}

}  // namespace

int main(int argc, char *argv[]) {
    Settings s;
    const Flag flags[] = {
        {"-input", Kind::Text, &s.input, "<string>, full path of input file (required); a name ending in .f2vcsr is read as a binary CSR."},
        {"-output", Kind::Text, &s.output, "<string>, directory (with trailing /) where the output file will be stored. (default: current directory)"},
        {"-batch", Kind::Integer, &s.batch, "<int>, size of minibatch. (default:384)"},
        {"-iter", Kind::Integer, &s.iter, "<int>, number of iteration. (default:1200)"},
        {"-threads", Kind::Integer, &s.threads, "<int>, accepted for compatibility (the force kernels run on the GPU)."},
        {"-dim", Kind::Integer, &s.dim, "<int>, size of embedding dimension, 1..512. (default:128)"},
        {"-nsamples", Kind::Integer, &s.nsamples, "<int>, number of negative samples. (default:5)"},
        {"-lr", Kind::Real, &s.lr, "<float>, learning rate of SGD. (default:0.02)"},
        {"-gamma", Kind::Real, &s.gamma, "<float>, accepted for compatibility (unused by options 1 and 5-11)."},
        {"-bs", Kind::Integer, &s.bs, "<int>, 1 = draw nsamples*batch negative samples per minibatch (options 5 and 6)."},
        {"-option", Kind::Integer, &s.option,
         "<int>, 1 Force2Vec (O(n^2) version: every vertex repelled by every other one, exact; one GPU; -nsamples and -lr are unused, -bs 1 is refused);\n"
         "        5 tForce2Vec (t-distribution + negative sampling), 6 sForce2Vec (sigmoid), 7 rForce2Vec (semi-random walk);\n"
         "        8..11 run the same three with the reference's AVX512 output names (8,11 -> 5; 9 -> 6; 10 -> 7). (default:5)"},
        {"-device", Kind::Integer, &s.device, "<int>, HIP device ordinal. (default:0)"},
        {"-seed", Kind::Integer, &s.seed, "<int>, srand() seed. (default:1)"},
        {"-cache", Kind::Integer, &s.cache, "<int>, 1 = keep / reuse the binary CSR <input>.f2vcsr."},
        {"-binout", Kind::Integer, &s.binout, "<int>, 1 = also write <output file>.bin, raw fp32 N x D (the scorers' binary embedding format)."},
        {"-init", Kind::Text, &s.init, "<string>, warm start: a text .embd (or, ending in .bin, raw fp32 N x D) of the run's N and -dim instead of the random initial embedding."},
        {"-notext", Kind::Integer, &s.notext, "<int>, 1 = skip the text .embd (use with -binout 1 for very large graphs)."},
        {"-gpus", Kind::Integer, &s.gpus, "<int>, number of GPUs (1..8): one process per GPU from -device on, minibatch rows sharded, rows exchanged over xGMI. (default:1)"},
        {"-samegpu", Kind::Integer, &s.samegpu, "<int>, 1 = all ranks of a -gpus run on device -device (self-test on a one-GPU machine)."},
        {"-fastrng", Kind::Integer, &s.fastrng, "<int>, 1 = NON-PARITY fast mode: initial embeddings and option-7 walks from a device-side RNG."},
        {"-loss", Kind::Integer, &s.loss, "<int>, k > 0: print \"Iteration:<epoch> :LOGLIKELIHOOD: <loss>\" after every k-th epoch and the last (the training objective, include/f2v.h; one GPU). (default:0)"},
        {"-nearest", Kind::Integer, &s.nearest, "<int>, k in 1..128: after training write <output file>.nn, one line per vertex \"v j1 s1 ... jk sk\" (its k nearest rows, self excluded), and print the precision@k against the graph (one GPU). (default:0)"},
        {"-nearest-lists", Kind::Integer, &s.nearest_lists, "<int>, L in 1..1024, at most the number of vertices: run the -nearest sweep through an inverted-file index (k-means of the trained matrix into L lists on the GPU, seeded by -seed; a query scores only the rows of the lists whose centroids are nearest) and print \"Index: lists <L> probes <P> candidates/query <c>\"; 0 = the exact search. (default:0)"},
        {"-nearest-probes", Kind::Integer, &s.nearest_probes, "<int>, p in 1..128: lists a query of a -nearest-lists sweep scores; with p >= L the result is the exact search's. (default:8)"},
        {"-nearest-iters", Kind::Integer, &s.nearest_iters, "<int>, most Lloyd iterations of the -nearest-lists k-means. (default:20)"},
        {"-nearest-check", Kind::Integer, &s.nearest_check, "<int>, s > 0: also print \"Recall@<k> against the exact search (<s> vertices): <r>\" of a -nearest-lists sweep over the vertices floor(i n / s), i < s. (default:0)"},
        {"-cluster", Kind::Integer, &s.cluster, "<int>, k in 1..1024: after training cluster the embedding with k-means on the GPU, write <output file>.clu, one line per vertex \"v label\" (0-based), and print the clustering's modularity on the graph (one GPU; seeded by -seed). (default:0)"},
        {"-cluster-iters", Kind::Integer, &s.cluster_iters, "<int>, most Lloyd iterations of a -cluster run. (default:300)"},
        {"-cluster-restarts", Kind::Integer, &s.cluster_restarts, "<int>, seeded runs of -cluster, the one of lowest inertia is kept (the scorer's n_init). (default:10)"},
        {"-classify", Kind::Text, &s.classify, "<string>, a labels file of lines \"vertex label\" (1-based vertex ids, labels 0..C-1, C <= 64): after training fit a one-vs-rest logistic regression on a share of the labelled vertices on the GPU and print \"Classify: frac <f> :F1-MICRO: <x> :F1-MACRO: <y>\", the mean F1 of the others in percent (one GPU; splits seeded by -seed)."},
        {"-classify-frac", Kind::Real, &s.classify_frac, "<float>, share of the labelled vertices a -classify split trains on, in (0, 1). (default:0.1)"},
        {"-classify-splits", Kind::Integer, &s.classify_splits, "<int>, seeded splits of -classify whose F1 values are averaged. (default:10)"},
        {"-separation", Kind::Text, &s.separation, "<string>, a labels file as -classify reads it (a vertex's first label counts, labels 0..1023), or \"kmeans\" for the clusters of this run's -cluster: after training print \"silhouette: <x> davies_bouldin: <y>\", how well the labelling separates in the embedding space (one GPU). A vertex the file does not name takes no part (the reference's script gives such vertices a cluster of their own, -1; on a fully labelled graph the two agree)."},
        {"-separation-sample", Kind::Integer, &s.separation_sample, "<int>, silhouette of that many labelled vertices chosen by -seed, each scored against all labelled vertices; 0 = every labelled vertex. (default:0)"},
        {"-layout", Kind::Integer, &s.layout, "<int>, d in 1..dim: after training write <output file>.lay, one line per vertex \"v y1 ... yd\" (1-based ids): the matrix projected onto its first d principal components on the GPU, and print \"TrustWorthiness: <t> Continuity: <c>\" of that picture and its explained-variance share (one GPU). (default:0)"},
        {"-layout-neighbours", Kind::Integer, &s.layout_neighbours, "<int>, k in 1..128, below half the number of vertices: the neighbourhood size of the -layout scores. (default:5)"},
        {"-layout-sample", Kind::Integer, &s.layout_sample, "<int>, score the -layout over that many vertices chosen by -seed, each ranked against all vertices; 0 = every vertex (O(N^2 dim) work). (default:0)"},
        {"-layout-method", Kind::Text, &s.layout_method, "<string>, pca or tsne: what -layout writes. tsne is the exact t-SNE of the matrix in d = 2 or 3 dimensions on the GPU (deterministic; started from the principal components as scikit-learn's init=\"pca\"; O(N^2) per iteration, at most 131072 vertices -- Engine.tsne(ids=...) lays out a subset of a larger graph). (default:pca)"},
        {"-layout-perplexity", Kind::Real, &s.layout_perplexity, "<float>, above 1 and at most 42, and 3 x perplexity below the number of vertices: the perplexity of -layout-method tsne. (default:30)"},
        {"-layout-iters", Kind::Integer, &s.layout_iters, "<int>, iterations of -layout-method tsne, the first 250 with early exaggeration. (default:1000)"},
        {"-foldin", Kind::Text, &s.foldin, "<string>, a file of lines \"<name> <nbr> <nbr> ...\" (1-based ids of existing vertices): after training -- or on -init <file> with -iter 0 -- give every line's new vertex a vector by running the option's update for it against the finished matrix on the GPU, and write <output file>.fold: \"<m> <dim>\", then per line the name and the vector (options 5, 6, 8, 9, 11; one GPU; samples seeded by -seed; -nsamples and -lr as in training)."},
        {"-foldin-iters", Kind::Integer, &s.foldin_iters, "<int>, epochs of a -foldin vertex. (default:300)"},
        {"-foldin-init", Kind::Text, &s.foldin_init, "<string>, initial vector of a -foldin vertex: mean (of its neighbours' vectors) | random. Under the sigmoid options (6, 9) a random start moves slowly: keep mean. (default:mean)"},
        {"-linkpredict", Kind::Text, &s.linkpredict, "<string>, hadamard | l1 | l2 | average: after training -- or on -init <file> with -iter 0 -- score link prediction as the reference does: the pair set (every edge once, -linkpredict-ratio times as many non-neighbours per vertex, shuffled by -seed) is built on the GPU, a logistic regression on that pair feature is fitted on its first part and predicts the rest; prints \"Link predictions(<Feature>): <frac> :Accuracy: <a> F1-macro: <m> F1-micro: <i>\", fractions of 1 (one GPU)."},
        {"-communities", Kind::Integer, &s.communities, "<int>, 1: after training (or on -init <file> with -iter 0) find the communities of the graph itself with the Louvain method on the GPU (integers only: the same result on every run), write <output file>.com, one line per vertex \"v label\" (0-based), and print \"Modularity: Louvain = <Q> Communities: <K> Levels: <L>\"; with -cluster also \"Agreement(kmeans, louvain): NMI <x> ARI <y>\", with -classify <labels> or -separation <labels file> also \"Agreement(labels, louvain): ...\" (a vertex's first label counts; one GPU; the graph must be symmetric). (default:0)"},
        {"-communities-levels", Kind::Integer, &s.communities_levels, "<int>, 1..65535: most levels of a -communities run. (default:32)"},
        {"-communities-seed", Kind::Integer, &s.communities_seed, "<int>, non-negative: the seed of the -communities sub-round classes. (default:1)"},
        {"-linkpredict-frac", Kind::Real, &s.linkpredict_frac, "<float>, above 0 and below 1: the share of the pair set that trains the -linkpredict model. (default:0.5)"},
        {"-linkpredict-ratio", Kind::Integer, &s.linkpredict_ratio, "<int>, 1..16: negatives per positive of a vertex in the -linkpredict pair set. (default:2)"},
        {"-holdout", Kind::Real, &s.holdout, "<float>, f in [0, 1): held-out link prediction. About that share of the edges is hidden before training (a hash of the pair seeded by -seed decides; every vertex keeps the edge of its lowest hash, so the share falls somewhat below f and no vertex loses all its neighbours; connectivity is not promised) and the run trains on the remaining graph: THE .embd IS THEN THE TRAINING GRAPH'S EMBEDDING, not the input graph's, and every other scorer flag of the run sees the training graph. Afterwards the hidden edges and -holdout-ratio times as many non-edges of the input graph per vertex are written to <output file>.held, one line \"u v y\" per pair (1-based ids, y = 1 for a hidden edge), ranked by the embedding's own similarity on the GPU, and \"Held-out link prediction(<metric>): <H> edges :AUC: <a> AP: <p>\" is printed (ROC-AUC with ties counted half, average precision); with -linkpredict <feature> the same line also for the decision values of the classifier, fitted on pairs of the training graph alone (one GPU; not with -foldin)."},
        {"-holdout-ratio", Kind::Integer, &s.holdout_ratio, "<int>, 0..16: non-edges per hidden edge of a vertex in the -holdout test set. (default:1)"},
        {"-holdout-keep", Kind::Text, &s.holdout_keep, "<string>, anchor | forest: what a -holdout split never hides. anchor: every vertex's edge of lowest hash (connectivity is not promised). forest: the spanning forest of greatest hashes, found on the GPU -- the training graph keeps exactly the components of the input graph, and no rule that keeps them hides more edges. (default:anchor)"},
        {"-components", Kind::Integer, &s.components, "<int>, 1: after the run (it needs no training: -iter 0 will do) find the connected components of the run's graph on the GPU, write <output file>.cc, one line per vertex \"v label\" (0-based; the label is the smallest id of the vertex's component), and print \"Components: <c> Largest: <s> Isolated: <z>\" (one GPU). (default:0)"},
        {"-holdout-ranks", Kind::Integer, &s.holdout_ranks, "<int>, with -holdout: the filtered rank of the hidden edges among ALL vertices, on the GPU. 0: off, -1: every hidden edge, s > 0: s of them, those of index floor(j H / s) of the H hidden edges. Each edge (u, v) is ranked from both ends by -holdout-metric, u itself and its training neighbours left out; prints \"Held-out ranks(<metric>): <P> pairs :MRR: <m> MeanRank: <r> Hits@1: <a> Hits@10: <b> Hits@50: <c> Hits@100: <d>\" (ties count half; hits as fractions of P) and writes <output file>.rank, one line \"u v greater equal\" per pair (1-based ids). (default:0)"},
        {"-holdout-metric", Kind::Text, &s.holdout_metric, "<string>, similarity that ranks the -holdout pairs: dot | l2 | cos. (default: l2 for options 1, 5, 8, 11, dot for the sigmoid options)"},
        {"-holdout-baselines", Kind::Integer, &s.holdout_baselines, "<int>, 1: with -holdout, also rank the same hidden edges and non-edges by the classic neighbourhood scores of the training graph, computed on the GPU -- common neighbours, Jaccard, Adamic-Adar, resource allocation, preferential attachment -- and print, after the embedding's line, \"Held-out baseline(<cn|jaccard|aa|ra|pa>): <H> edges :AUC: <a> AP: <p>\" for each: the yardstick the embedding's AUC and AP are read against. (default:0)"},
        {"-metric", Kind::Text, &s.metric, "<string>, similarity of -nearest: dot | l2 | cos. (default: l2 for options 5, 8, 11, dot for the sigmoid options)"},
    };
    const size_t nflags = sizeof flags / sizeof flags[0];
    for (int p = 1; p < argc; p++) {
        if (!strcmp(argv[p], "-h")) {
            usage(flags, nflags);
            return 1;  // Test/Force2Vec.cpp:112-115
        }
        for (size_t k = 0; k < nflags && p + 1 < argc; k++) {
            if (strcmp(argv[p], flags[k].name)) continue;
            const char *v = argv[++p];
            if (flags[k].kind == Kind::Text) *static_cast<std::string *>(flags[k].target) = v;
            else if (flags[k].kind == Kind::Integer) *static_cast<long *>(flags[k].target) = atol(v);
            else *static_cast<double *>(flags[k].target) = atof(v);
            break;
        }
    }
    if (s.input.empty()) {
        printf("Valid input file needed!...\n");  // Test/Force2Vec.cpp:117-120
        return 1;
    }
    const Variant *variant = nullptr;
    for (const Variant &v : kVariants)
        if (v.option == s.option) variant = &v;
    if (!variant) {
        printf("This build implements option 1 (exact all-pairs Force2Vec) and options 5 to 11 (the negative-sampling force kernels); option %ld is out of scope.\n", s.option);
        return 1;
    }
    if (s.batch <= 0 || s.dim <= 0 || s.iter < 0 || s.nsamples < 0) {
        printf("-batch and -dim must be positive, -iter and -nsamples non-negative.\n");
        return 1;
    }
    if (s.gpus < 1 || s.gpus > F2V_PUSH_MAX_RANKS) {
        printf("-gpus must be 1..%d.\n", F2V_PUSH_MAX_RANKS);
        return 1;
    }
    if (s.option == 1 && s.gpus > 1) {
        printf("-option 1 is not available with -gpus > 1 (the exact all-pairs method runs on one GPU).\n");
        return 1;
    }
    if (s.option == 1 && s.bs != 0) {
        printf("-option 1 has no -bs 1 variant (the exact all-pairs method draws no samples).\n");
        return 1;
    }
    if (s.loss < 0 || s.loss > 0x7FFFFFFF) {
        printf("-loss must be a non-negative number of epochs.\n");
        return 1;
    }
    if (s.loss > 0 && s.gpus > 1) {
        printf("-loss is not available with -gpus > 1 (a rank does not hold the whole matrix between minibatches).\n");
        return 1;
    }
    if (s.nearest < 0 || s.nearest > F2V_NEAREST_MAX_K) {
        printf("-nearest must be 0..%d.\n", F2V_NEAREST_MAX_K);
        return 1;
    }
    if (s.metric.empty()) s.metric = (s.option == 1 || s.option == 5 || s.option == 8 || s.option == 11) ? "l2" : "dot";
    const int metric = s.metric == "dot" ? F2V_SIM_DOT : s.metric == "l2" ? F2V_SIM_L2 : s.metric == "cos" ? F2V_SIM_COSINE : -1;
    if (metric < 0) {
        printf("-metric must be dot, l2 or cos.\n");
        return 1;
    }
    if (s.nearest_lists < 0 || s.nearest_lists > F2V_INDEX_MAX_LISTS) {
        printf("-nearest-lists must be 0..%d.\n", F2V_INDEX_MAX_LISTS);
        return 1;
    }
    if (s.nearest_probes < 0 || s.nearest_probes > F2V_INDEX_MAX_PROBES) {
        printf("-nearest-probes must be 1..%d.\n", F2V_INDEX_MAX_PROBES);
        return 1;
    }
    if (s.nearest_iters < 0 || s.nearest_iters > 0x7FFFFFFF || s.nearest_check < 0 || s.nearest_check > 0x7FFFFFFF) {
        printf("-nearest-iters and -nearest-check must be non-negative.\n");
        return 1;
    }
    if (s.nearest == 0 && (s.nearest_lists > 0 || s.nearest_probes > 0 || s.nearest_check > 0)) {
        printf("-nearest-lists, -nearest-probes and -nearest-check need -nearest.\n");
        return 1;
    }
    if (s.nearest_lists == 0 && (s.nearest_probes > 0 || s.nearest_check > 0)) {
        printf("-nearest-probes and -nearest-check need -nearest-lists.\n");
        return 1;
    }
    if (s.nearest > 0 && s.gpus > 1) {
        printf("-nearest is not available with -gpus > 1 (it queries one GPU's matrix).\n");
        return 1;
    }
    if (s.cluster < 0 || s.cluster > F2V_KMEANS_MAX_K) {
        printf("-cluster must be 0..%d.\n", F2V_KMEANS_MAX_K);
        return 1;
    }
    if (s.cluster > 0 && (s.cluster_restarts < 1 || s.cluster_restarts > 0x7FFFFFFF)) {
        printf("-cluster-restarts must be at least 1.\n");
        return 1;
    }
    if (s.cluster > 0 && (s.cluster_iters < 0 || s.cluster_iters > 0x7FFFFFFF)) {
        printf("-cluster-iters must be a non-negative number of iterations.\n");
        return 1;
    }
    if (s.cluster > 0 && s.gpus > 1) {
        printf("-cluster is not available with -gpus > 1 (it clusters one GPU's matrix).\n");
        return 1;
    }
    if (!s.classify.empty() && !(s.classify_frac > 0.0 && s.classify_frac < 1.0)) {
        printf("-classify-frac must be above 0 and below 1.\n");
        return 1;
    }
    if (!s.classify.empty() && (s.classify_splits < 1 || s.classify_splits > 0x7FFFFFFF)) {
        printf("-classify-splits must be at least 1.\n");
        return 1;
    }
    if (!s.classify.empty() && s.gpus > 1) {
        printf("-classify is not available with -gpus > 1 (it scores one GPU's matrix).\n");
        return 1;
    }
    if (s.separation == "kmeans" && s.cluster <= 0) {
        printf("-separation kmeans scores the clusters of -cluster <k>: give it too.\n");
        return 1;
    }
    if (s.separation_sample < 0 || s.separation_sample > 0x7FFFFFFF) {
        printf("-separation-sample must be a non-negative number of vertices.\n");
        return 1;
    }
    if (!s.separation.empty() && s.gpus > 1) {
        printf("-separation is not available with -gpus > 1 (it scores one GPU's matrix).\n");
        return 1;
    }
    if (s.layout < 0 || s.layout > s.dim) {
        printf("-layout must be 0..-dim (%ld).\n", s.dim);
        return 1;
    }
    if (s.layout_neighbours < 1 || s.layout_neighbours > F2V_NEAREST_MAX_K) {
        printf("-layout-neighbours must be 1..%d.\n", F2V_NEAREST_MAX_K);
        return 1;
    }
    if (s.layout_sample < 0 || s.layout_sample > 0x7FFFFFFF) {
        printf("-layout-sample must be a non-negative number of vertices.\n");
        return 1;
    }
    if (s.layout_method != "pca" && s.layout_method != "tsne") {
        printf("-layout-method must be pca or tsne.\n");
        return 1;
    }
    const bool tsne = s.layout_method == "tsne";
    if (tsne && s.layout != 0 && s.layout != 2 && s.layout != 3) {
        printf("-layout with -layout-method tsne must be 2 or 3.\n");
        return 1;
    }
    if (tsne && !(s.layout_perplexity > 1.0 && 3.0 * s.layout_perplexity < F2V_NEAREST_MAX_K + 1.0)) {
        printf("-layout-perplexity must be above 1 with at most %d neighbours (3 x perplexity).\n", F2V_NEAREST_MAX_K);
        return 1;
    }
    if (tsne && (s.layout_iters < 1 || s.layout_iters > 0x7FFFFFFF)) {
        printf("-layout-iters must be at least 1.\n");
        return 1;
    }
    if (s.layout > 0 && s.gpus > 1) {
        printf("-layout is not available with -gpus > 1 (it projects and scores one GPU's matrix).\n");
        return 1;
    }
    const int foldin_init = s.foldin_init == "mean" ? F2V_FOLD_INIT_MEAN : s.foldin_init == "random" ? F2V_FOLD_INIT_RANDOM : -1;
    if (!s.foldin.empty() && foldin_init < 0) {
        printf("-foldin-init must be mean or random.\n");
        return 1;
    }
    if (!s.foldin.empty() && (s.foldin_iters < 0 || s.foldin_iters > 0x7FFFFFFF)) {
        printf("-foldin-iters must be a non-negative number of epochs.\n");
        return 1;
    }
    if (!s.foldin.empty() && (s.option == 1 || s.option == 7 || s.option == 10)) {
        printf("-foldin is available with options 5, 6, 8, 9 and 11 (a new vertex has no walks, and option 1 repels it from every vertex).\n");
        return 1;
    }
    if (!s.foldin.empty() && s.gpus > 1) {
        printf("-foldin is not available with -gpus > 1 (it reads one GPU's matrix).\n");
        return 1;
    }
    const int linkpredict_feature = s.linkpredict == "hadamard" ? F2V_PAIR_HADAMARD : s.linkpredict == "l1" ? F2V_PAIR_L1 : s.linkpredict == "l2" ? F2V_PAIR_L2 : s.linkpredict == "average" ? F2V_PAIR_AVERAGE : -1;
    if (!s.linkpredict.empty() && linkpredict_feature < 0) {
        printf("-linkpredict must be hadamard, l1, l2 or average.\n");
        return 1;
    }
    if (!s.linkpredict.empty() && !(s.linkpredict_frac > 0.0 && s.linkpredict_frac < 1.0)) {
        printf("-linkpredict-frac must be above 0 and below 1.\n");
        return 1;
    }
    if (!s.linkpredict.empty() && (s.linkpredict_ratio < 1 || s.linkpredict_ratio > 16)) {
        printf("-linkpredict-ratio must be 1..16.\n");
        return 1;
    }
    if (s.communities < 0 || s.communities > 1) {
        printf("-communities must be 0 or 1.\n");
        return 1;
    }
    if (s.communities && (s.communities_levels < 1 || s.communities_levels > 65535)) {
        printf("-communities-levels must be 1..65535.\n");
        return 1;
    }
    if (s.communities && s.communities_seed < 0) {
        printf("-communities-seed must be a non-negative number.\n");
        return 1;
    }
    if (s.communities && s.gpus > 1) {
        printf("-communities is not available with -gpus > 1 (it runs on one GPU's copy of the graph).\n");
        return 1;
    }
    const bool holdout = s.holdout != -1.0;
    if (holdout && !(s.holdout >= 0.0 && s.holdout < 1.0)) {
        printf("-holdout must be at least 0 and below 1.\n");
        return 1;
    }
    if (holdout && (s.holdout_ratio < 0 || s.holdout_ratio > 16)) {
        printf("-holdout-ratio must be 0..16.\n");
        return 1;
    }
    if (s.holdout_metric.empty()) s.holdout_metric = (s.option == 1 || s.option == 5 || s.option == 8 || s.option == 11) ? "l2" : "dot";
    const int holdout_metric = s.holdout_metric == "dot" ? F2V_SIM_DOT : s.holdout_metric == "l2" ? F2V_SIM_L2 : s.holdout_metric == "cos" ? F2V_SIM_COSINE : -1;
    if (holdout && holdout_metric < 0) {
        printf("-holdout-metric must be dot, l2 or cos.\n");
        return 1;
    }
    if (!s.holdout_keep.empty() && s.holdout_keep != "anchor" && s.holdout_keep != "forest") {
        printf("-holdout-keep must be anchor or forest.\n");
        return 1;
    }
    if (!s.holdout_keep.empty() && !holdout) {
        printf("-holdout-keep needs -holdout (it chooses what the split protects).\n");
        return 1;
    }
    if (s.holdout_baselines < 0 || s.holdout_baselines > 1) {
        printf("-holdout-baselines must be 0 or 1.\n");
        return 1;
    }
    if (s.holdout_baselines && !holdout) {
        printf("-holdout-baselines needs -holdout (it scores the pairs that the split hides).\n");
        return 1;
    }
    if (s.holdout_ranks < -1 || s.holdout_ranks > 0x7FFFFFFF) {
        printf("-holdout-ranks must be -1 (every hidden edge), 0 (off) or a number of hidden edges.\n");
        return 1;
    }
    if (s.holdout_ranks && !holdout) {
        printf("-holdout-ranks needs -holdout (it ranks the edges that the split hides).\n");
        return 1;
    }
    if (s.components < 0 || s.components > 1) {
        printf("-components must be 0 or 1.\n");
        return 1;
    }
    if (s.components && s.gpus > 1) {
        printf("-components is not available with -gpus > 1 (it runs on one GPU's copy of the graph).\n");
        return 1;
    }
    if (holdout && s.gpus > 1) {
        printf("-holdout is not available with -gpus > 1 (it splits and scores on one GPU).\n");
        return 1;
    }
    if (holdout && !s.foldin.empty()) {
        printf("-holdout is not available with -foldin (a new vertex's neighbours are edges of the input graph, which the run did not train on).\n");
        return 1;
    }
    std::vector<VALUETYPE> seconds;
    int rank = 0;
    std::string meet;  // directory the ranks of a -gpus run meet in
    try {
        CSRGraph graph;
        SetInputMatricesAsCSR(graph, s.input, s.cache != 0);  // host only: read once, inherited by the forked ranks
        if (tsne && s.layout > 0 && graph.rows > 131072)
            throw std::runtime_error("-layout-method tsne lays out at most 131072 vertices (every iteration visits all pairs): lay out a subset with Engine.tsne(ids=...), or use -layout-method pca");
        std::vector<pid_t> kids;
        if (s.gpus > 1) {
            char tmpl[] = "/tmp/f2v_ranks_XXXXXX";
            if (!mkdtemp(tmpl)) throw std::runtime_error("cannot create a meeting directory under /tmp");
            meet = tmpl;
            fflush(nullptr);
            // no HIP call has been made yet: every rank initialises its own GPU after the fork
            for (int r = 1; r < s.gpus; r++) {
                const pid_t pid = fork();
                if (pid < 0) throw std::runtime_error("fork failed");
                if (pid == 0) { rank = r; kids.clear(); break; }
                kids.push_back(pid);
            }
        }
        int rc_mine = 0;
        try {
            Holdout split;
            if (holdout) SplitForHoldout(graph, s.holdout, (uint32_t)s.holdout_ratio, (uint64_t)s.seed, (int)s.device, split, s.holdout_keep == "forest");
            algorithms algo(holdout ? split.train : graph, s.input, s.output, (INDEXTYPE)s.dim, (VALUETYPE)s.gamma, (INDEXTYPE)s.batch, (int)s.device + (s.samegpu ? 0 : rank));
            algo.binary_output = s.binout != 0;
            algo.text_output = s.notext == 0;
            algo.init_path = s.init;
            if (s.fastrng && f2v_set_param(algo.h, "fast_rng", 1) != F2V_OK) throw std::runtime_error(f2v_last_error());
            if (s.loss > 0 && f2v_set_param(algo.h, "loss_every", s.loss) != F2V_OK) throw std::runtime_error(f2v_last_error());
            algo.srand((unsigned)s.seed);
            if (s.gpus > 1) algo.join_ranks(rank, (int)s.gpus, meet);
            if (rank == 0) std::cout << "Running: " << variant->name << std::endl;
            auto method = (s.bs != 0 && variant->with_bs) ? variant->with_bs : variant->plain;
            if (!method) seconds = algo.AlgoForce2Vec((INDEXTYPE)s.iter, (INDEXTYPE)s.threads, (INDEXTYPE)s.batch);
            else seconds = (algo.*method)((INDEXTYPE)s.iter, (INDEXTYPE)s.threads, (INDEXTYPE)s.batch, (INDEXTYPE)s.nsamples, (VALUETYPE)s.lr);
            if (s.loss > 0 && rank == 0) {  // the reference's commented-out print (sample/algorithms.cpp:645), from the run's log
                uint32_t count = 0;
                if (f2v_train_losses(algo.h, nullptr, nullptr, 0, &count) != F2V_OK) throw std::runtime_error(f2v_last_error());
                std::vector<uint32_t> epochs(count);
                std::vector<double> values(3 * (size_t)count);
                if (f2v_train_losses(algo.h, epochs.data(), values.data(), count, &count) != F2V_OK) throw std::runtime_error(f2v_last_error());
                for (uint32_t m = 0; m < count; m++) std::cout << "Iteration:" << epochs[m] << " :LOGLIKELIHOOD: " << values[3 * m] << std::endl;
            }
            if (s.nearest > 0 && rank == 0) algo.writeNearest((uint32_t)s.nearest, metric, s.metric.c_str(), (uint32_t)s.nearest_lists, (uint32_t)(s.nearest_probes ? s.nearest_probes : 8), (uint32_t)s.nearest_iters, (uint64_t)s.seed, (uint32_t)s.nearest_check);
            if (s.cluster > 0 && rank == 0) algo.writeClusters((uint32_t)s.cluster, (uint32_t)s.cluster_iters, (uint32_t)s.cluster_restarts, (uint64_t)s.seed);
            if (!s.classify.empty() && rank == 0) algo.classify(s.classify, s.classify_frac, (uint32_t)s.classify_splits, (uint64_t)s.seed);
            if (!s.separation.empty() && rank == 0) algo.separation(s.separation, (uint32_t)s.separation_sample, (uint64_t)s.seed);
            if (s.layout > 0 && rank == 0)
                algo.layout((uint32_t)s.layout, (uint32_t)s.layout_neighbours, (uint32_t)s.layout_sample, (uint64_t)s.seed, tsne, s.layout_perplexity, (uint32_t)s.layout_iters);
            if (!s.foldin.empty() && rank == 0) algo.foldIn(s.foldin, (int)s.option, (uint32_t)s.foldin_iters, (INDEXTYPE)s.nsamples, (VALUETYPE)s.lr, foldin_init, (uint64_t)s.seed);
            if (!s.linkpredict.empty() && rank == 0) algo.linkPredict(linkpredict_feature, s.linkpredict_frac, (uint32_t)s.linkpredict_ratio, (uint64_t)s.seed);
            if (holdout && rank == 0)
                algo.heldOut(split, holdout_metric, s.holdout_metric.c_str(), s.linkpredict.empty() ? -1 : linkpredict_feature, (uint32_t)s.linkpredict_ratio, (uint64_t)s.seed);
            if (holdout && s.holdout_baselines && rank == 0) algo.heldOutBaselines(split);
            if (holdout && s.holdout_ranks && rank == 0) algo.heldOutRanks(split, holdout_metric, s.holdout_metric.c_str(), s.holdout_ranks);
            if (s.components && rank == 0) algo.writeComponents();
            if (s.communities && rank == 0)
                algo.writeCommunities((uint32_t)s.communities_levels, (uint64_t)s.communities_seed,
                                      !s.separation.empty() && s.separation != "kmeans" ? s.separation : s.classify);
            const double t = algo.gpu_train_seconds;
            if (rank == 0 && s.gpus == 1)
                printf("GPU epoch loop: %.6f s, %.4g nnz/s, %.1f GB/s algorithmic\n", t, t > 0 ? algo.stats.nnz / t : 0.0,
                       t > 0 ? algo.stats.algorithmic_bytes / t * 1e-9 : 0.0);
            else if (rank == 0)
                printf("GPU epoch loop: %.6f s, %.4g nnz/s on %ld GPUs\n", t, t > 0 ? (double)graph.nnz * (double)s.iter / t : 0.0, s.gpus);
        } catch (const std::exception &e) {
            fprintf(stderr, "Force2Vec%s: %s\n", s.gpus > 1 ? (" [rank " + std::to_string(rank) + "]").c_str() : "", e.what());
            rc_mine = 2;
        }
        if (rank != 0) _exit(rc_mine);  // a forked rank: nothing of the parent's to unwind
        for (pid_t pid : kids) {
            int st = 0;
            if (waitpid(pid, &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) rc_mine = 2;
        }
        if (!meet.empty()) {
            for (int r = 0; r < s.gpus; r++) (void)remove((meet + "/f2v_export." + std::to_string(r)).c_str());
            (void)rmdir(meet.c_str());
        }
        if (rc_mine) return rc_mine;
    } catch (const std::exception &e) {
        fprintf(stderr, "Force2Vec: %s\n", e.what());
        return 2;
    }
    // one line per run appended to ./Results.txt, in the reference's format (Test/Force2Vec.cpp:191-198)
    std::ofstream log("Results.txt", std::ofstream::app);
    log << "Algo:" << variant->name << "\tInit:RAND\tIteration:" << s.iter << "\tNumofthreads:" << s.threads << "\tBatchSize:" << s.batch
        << "\tDimension:" << s.dim << "\tTime(sec.):" << seconds[0] << "\t" << std::endl;
    return 0;
}
