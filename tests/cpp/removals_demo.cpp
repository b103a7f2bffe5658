// tests/cpp/removals_demo.cpp — selection of the vertices to remove through the C++ façade (include/spg_graph_wrapper.hpp:
// selectRemovals, include/spg.h: spg_graph_select_removals), tests/test_cpp_removals.py.
//
//   removals_demo <graph.g2o> <radius> <max_angle> <keep_id> <order> <out.txt>
//                                           order = hash | oldest | newest; keep_id < 0: nothing forced; writes
//                                           "removed representative rep_dist" per removed vertex, in order
//   removals_demo                           usage, exit 2
#include <cstdio>
#include <cstdlib>
#include <string>

#include "spg_graph_wrapper.hpp"

int main(int argc, char **argv) {
    if (argc < 7) {
        std::fprintf(stderr, "usage: removals_demo <graph.g2o> <radius> <max_angle> <keep_id> <hash|oldest|newest> <out.txt>\n");
        return 2;
    }
    try {
        spg::GraphWrapperHIP g(argv[1]);
        const double radius = std::atof(argv[2]), max_angle = std::atof(argv[3]);
        const int keep_id = std::atoi(argv[4]);
        const std::string order = argv[5];
        std::vector<int> keep;
        if (keep_id >= 0) keep.push_back(keep_id);
        std::vector<double> priority;
        if (order != "hash") {
            const int n = spg_graph_num_vertices(g.handle());
            std::vector<int32_t> ids((size_t)n);
            std::vector<double> poses((size_t)n * 7);
            if (spg_graph_get_vertices(g.handle(), ids.data(), poses.data()) < 0) return 6;
            std::sort(ids.begin(), ids.end());
            for (int32_t id : ids) priority.push_back(order == "oldest" ? -(double)id : (double)id);
        }
        spg::GraphWrapperHIP::RemovalResult R = g.selectRemovals(radius, max_angle, keep, priority);
        FILE *f = std::fopen(argv[6], "w");
        if (!f) return 4;
        for (size_t i = 0; i < R.removed.size(); i++) std::fprintf(f, "%d %d %.17g\n", R.removed[i], R.representative[i], R.rep_dist[i]);
        std::fclose(f);
        const spg_removal_stats &st = R.stats;
        if ((int)R.removed.size() != st.n_removed || st.n_kept + st.n_removed != st.n_live || st.n_forced != (int)keep.size()) {
            std::printf("the stats disagree with the result\n");
            return 3;
        }
        bool threw = false;
        try {
            g.selectRemovals(0.0);   // radius <= 0: SPG_EINVAL, reported as an exception
        } catch (const std::exception &) {
            threw = true;
        }
        std::printf("%zu of %d vertices removed, %d kept (%d forced), %d rounds, %lld distance tests over %d cells (largest %d) in %lld slots; %.3f ms\n",
                    R.removed.size(), st.n_live, st.n_kept, st.n_forced, st.rounds, (long long)st.pairs_tested, st.n_cells, st.max_cell_population,
                    (long long)st.table_slots, st.device_seconds * 1e3);
        if (!threw) { std::printf("radius = 0 was accepted\n"); return 5; }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    std::printf("removals ok\n");
    return 0;
}
