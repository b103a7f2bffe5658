// tests/cpp/outlier_demo.cpp — greedy data snooping through the C++ façade (include/spg_graph_wrapper.hpp: detectOutliers /
// rejectOutliers, include/spg.h: spg_graph_detect_outliers), tests/test_outlier_detection.py.
//
//   outlier_demo <graph.g2o> <k> <min_stat> <out.txt>   candidates: every third live edge of the graph (0, 3, 6, ... in
//                                                       the order of edges()); flags up to k of them, writes "index stat"
//                                                       per line in order, then "r index redundancy status" per
//                                                       candidate, and removes the flagged edges from the graph
//   outlier_demo                                        usage, exit 2
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "spg_graph_wrapper.hpp"

int main(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: outlier_demo <graph.g2o> <k> <min_stat> <out.txt>\n");
        return 2;
    }
    try {
        spg::GraphWrapperHIP g(argv[1]);
        const int k = std::atoi(argv[2]);
        const double min_stat = std::atof(argv[3]);
        const int ne = g.numEdges();
        std::vector<int> idx;
        for (int e = 0; e < ne; e += 3) idx.push_back(e);
        spg_outlier_stats st{};
        spg::GraphWrapperHIP::OutlierResult R = g.rejectOutliers(idx, k, min_stat, 0.0, -1, &st);
        FILE *f = std::fopen(argv[4], "w");
        if (!f) return 4;
        for (size_t t = 0; t < R.flagged.size(); t++) std::fprintf(f, "%d %.17g\n", R.flagged[t], R.stat[t]);
        for (size_t i = 0; i < R.status.size(); i++) std::fprintf(f, "r %zu %.17g %d\n", i, R.redundancy[i], R.status[i]);
        std::fclose(f);
        int marked = 0;
        for (int s : R.status) marked += s == SPG_OUTLIER_FLAGGED;
        if (marked != (int)R.flagged.size() || st.rounds != (int)R.flagged.size()) { std::printf("status and rounds disagree with the result\n"); return 3; }
        if (g.numEdges() != ne - (int)R.flagged.size()) { std::printf("the flagged edges are still in the graph\n"); return 6; }
        bool threw = false;
        try {
            g.detectOutliers(idx, -1);   // k < 0 (and indices now out of range): SPG_EINVAL, reported as an exception
        } catch (const std::exception &) {
            threw = true;
        }
        std::printf("%zu of %zu edges flagged over %d endpoints in %d rounds, %.2f ms (detection %.2f ms)\n", R.flagged.size(), idx.size(), st.endpoints,
                    st.rounds, st.solve.cov.device_seconds * 1e3, st.detect_seconds * 1e3);
        if (!threw) { std::printf("k = -1 was accepted\n"); return 5; }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    std::printf("outliers ok\n");
    return 0;
}
