// tests/cpp/prune_demo.cpp — greedy edge pruning through the C++ façade (include/spg_graph_wrapper.hpp: pruneEdges,
// include/spg.h: spg_graph_prune_candidates / spg_graph_remove_edges), tests/test_edge_pruning.py.
//
//   prune_demo <graph.g2o> <k> <out.txt>   candidates: every third live edge of the graph (0, 3, 6, ... in the order of
//                                          edges()); prunes k of them, writes "index loss kld" per line in order and
//                                          removes the pruned edges from the graph
//   prune_demo                             usage, exit 2
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "spg_graph_wrapper.hpp"

int main(int argc, char **argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: prune_demo <graph.g2o> <k> <out.txt>\n");
        return 2;
    }
    try {
        spg::GraphWrapperHIP g(argv[1]);
        const int k = std::atoi(argv[2]);
        const int ne = g.numEdges();
        std::vector<int> idx;
        for (int e = 0; e < ne; e += 3) idx.push_back(e);
        spg_prune_stats st;
        spg::GraphWrapperHIP::PruneResult R = g.pruneEdges(idx, k, 0.0, 0.0, 0.0, -1, &st);
        FILE *f = std::fopen(argv[3], "w");
        if (!f) return 4;
        for (size_t t = 0; t < R.pruned.size(); t++) std::fprintf(f, "%d %.17g %.17g\n", R.pruned[t], R.cond_loss[t], R.kld[t]);
        std::fclose(f);
        int marked = 0;
        for (int s : R.status) marked += s == SPG_PRUNE_PRUNED;
        if (marked != (int)R.pruned.size() || st.rounds != (int)R.pruned.size()) { std::printf("status and rounds disagree with the result\n"); return 3; }
        if (g.numEdges() != ne - (int)R.pruned.size()) { std::printf("the pruned edges are still in the graph\n"); return 6; }
        bool threw = false;
        try {
            g.pruneCandidates(idx, -1);   // k < 0 (and indices now out of range): SPG_EINVAL, reported as an exception
        } catch (const std::exception &) {
            threw = true;
        }
        std::printf("%zu of %zu edges pruned over %d endpoints in %d rounds, %.2f ms (pruning %.2f ms)\n", R.pruned.size(), idx.size(), st.endpoints,
                    st.rounds, st.solve.cov.device_seconds * 1e3, st.prune_seconds * 1e3);
        if (!threw) { std::printf("k = -1 was accepted\n"); return 5; }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    std::printf("pruning ok\n");
    return 0;
}
