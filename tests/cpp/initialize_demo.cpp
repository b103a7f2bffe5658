// tests/cpp/initialize_demo.cpp — initialize() of the C++ façade (include/spg_graph_wrapper.hpp) driven from C++
// (tests/test_initialize_facade.py).
//
//   initialize_demo <graph.g2o>   every estimate but the first reset to the identity, initialize() in both modes, then
//                                 optimize(): the chi2 of optimize() from the file's own poses is reached again
//   initialize_demo               usage, exit 2
#include <cmath>
#include <cstdio>
#include <vector>

#include "spg_graph_wrapper.hpp"

static void forget_estimates(spg::GraphWrapperHIP &g) {
    std::vector<int> ids;
    bool is2d = true;
    for (const spg::GraphWrapper::Vertex *v : g.vertices()) { ids.push_back(v->id()); is2d = v->is2d(); }
    for (size_t i = 1; i < ids.size(); i++) g.setEstimate(ids[i], spg::IsometryXd(is2d));
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: initialize_demo <graph.g2o>\n");
        return 2;
    }
    try {
        spg::GraphWrapperHIP ref(argv[1]);
        const spg_optimize_stats want = ref.optimizeFromId(-1);
        for (int method : {SPG_INIT_SPANNING_TREE, SPG_INIT_CHORDAL}) {
            spg::GraphWrapperHIP g(argv[1]);
            forget_estimates(g);
            const double lost = g.chi2();
            const spg_init_stats st = g.initialize(method);
            if (st.method != method || st.n_vertices != (int)g.vertices().size() || st.edges_used <= 0) { std::printf("method %d: stats do not describe the call\n", method); return 3; }
            if (st.chi2_before != lost || st.chi2_after != g.chi2()) { std::printf("method %d: chi2_before / chi2_after are not chi2()\n", method); return 4; }
            // (a tree accumulates the noise of its edges: only the chordal estimate has to beat the identity poses)
            if (method == SPG_INIT_CHORDAL && !(st.chi2_after < st.chi2_before)) { std::printf("chordal: chi2 %g -> %g\n", st.chi2_before, st.chi2_after); return 5; }
            if (method == SPG_INIT_CHORDAL) {
                if (st.degenerate != 0 || st.supernodes <= 0 || !(st.device_seconds > 0)) { std::printf("chordal: degenerate %d, supernodes %d\n", st.degenerate, st.supernodes); return 6; }
                const spg_optimize_stats got = g.optimizeFromId(-1);
                if (!(std::fabs(got.chi2_final - want.chi2_final) <= 1e-9 * want.chi2_final)) {
                    std::printf("optimize() after initialize(): chi2 %.17g, from the file's poses %.17g\n", got.chi2_final, want.chi2_final);
                    return 7;
                }
                std::printf("chordal: chi2 %.6g -> %.6g -> %.9g in %d iterations (file poses: %.9g)\n", st.chi2_before, st.chi2_after, got.chi2_final,
                            got.iterations, want.chi2_final);
            } else {
                std::printf("tree: depth %d, chi2 %.6g -> %.6g\n", st.tree_depth, st.chi2_before, st.chi2_after);
            }
        }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    std::printf("initialize ok\n");
    return 0;
}
