// tests/cpp/propose_demo.cpp — proposal of loop-closure candidates through the C++ façade (include/spg_graph_wrapper.hpp:
// proposeCandidates, include/spg.h: spg_graph_propose_candidates), tests/test_cpp_propose.py.
//
//   propose_demo <graph.g2o> <search_radius> <min_id_gap> <max_per_vertex> <range> <out.txt>
//                                           every vertex a query, no angle test, z_max = 2; writes "id_a id_b dist angle" per
//                                           kept pair (and " sigma zscore" with range > 0), in order
//   propose_demo                            usage, exit 2
#include <cstdio>
#include <cstdlib>

#include "spg_graph_wrapper.hpp"

int main(int argc, char **argv) {
    if (argc < 7) {
        std::fprintf(stderr, "usage: propose_demo <graph.g2o> <search_radius> <min_id_gap> <max_per_vertex> <range> <out.txt>\n");
        return 2;
    }
    try {
        spg::GraphWrapperHIP g(argv[1]);
        const double radius = std::atof(argv[2]), range = std::atof(argv[5]);
        const int gap = std::atoi(argv[3]), m = std::atoi(argv[4]);
        spg::GraphWrapperHIP::ProposeResult R = g.proposeCandidates(radius, 0.0, gap, m, {}, range, 2.0);
        FILE *f = std::fopen(argv[6], "w");
        if (!f) return 4;
        for (size_t i = 0; i < R.ij.size(); i++) {
            std::fprintf(f, "%d %d %.17g %.17g", R.ij[i].first, R.ij[i].second, R.dist[i], R.angle[i]);
            if (range > 0.0) std::fprintf(f, " %.17g %.17g", R.sigma[i], R.zscore[i]);
            std::fprintf(f, "\n");
        }
        std::fclose(f);
        const spg_propose_stats &st = R.stats;
        if ((long long)R.ij.size() != (long long)st.n_gated || st.n_gated > st.n_kept || st.n_kept > st.n_qualifying) {
            std::printf("the stats disagree with the result\n");
            return 3;
        }
        bool threw = false;
        try {
            g.proposeCandidates(0.0);   // search_radius <= 0: SPG_EINVAL, reported as an exception
        } catch (const std::exception &) {
            threw = true;
        }
        std::printf("%zu pairs of %lld kept and %lld qualifying, %lld distance tests over %d cells (largest %d) in %lld slots; search %.3f ms, "
                    "%d covariance columns\n", R.ij.size(), (long long)st.n_kept, (long long)st.n_qualifying, (long long)st.pairs_tested, st.n_cells,
                    st.max_cell_population, (long long)st.table_slots, st.device_seconds * 1e3, st.solve.columns);
        if (!threw) { std::printf("search_radius = 0 was accepted\n"); return 5; }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    std::printf("proposal ok\n");
    return 0;
}
