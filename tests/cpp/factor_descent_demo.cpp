// tests/cpp/factor_descent_demo.cpp — the factor-descent members of the C++ façade (include/spg_graph_wrapper.hpp:
// setFactorDescent / factorDescent / setFactorDescentParams, SPG_FLAG_NFR_FACTOR_DESCENT) driven from C++
// (tests/test_factor_descent.py).
//
//   factor_descent_demo <graph.g2o>   the odd vertices removed under Subgraph(0.5): interior point, then factor descent
//   factor_descent_demo               usage, exit 2
#include <cmath>
#include <cstdio>
#include <vector>

#include "spg_graph_wrapper.hpp"

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: factor_descent_demo <graph.g2o>\n");
        return 2;
    }
    try {
        spg::SparsityOptions o;
        o.topology = spg::SparsityOptions::Subgraph;
        o.chordRatio = 0.5;
        o.linPoint = spg::SparsityOptions::Global;
        double kld[2] = {0, 0};
        int edges[2] = {0, 0};
        for (int pass = 0; pass < 2; pass++) {
            spg::GraphWrapperHIP g(argv[1]);
            if (g.factorDescent()) { std::printf("factor descent is on by default\n"); return 3; }
            g.setFactorDescent(pass == 1);
            if (g.factorDescent() != (pass == 1)) { std::printf("factorDescent() does not return the setting\n"); return 4; }
            if (pass == 1) g.setFactorDescentParams(0.0, 0);      // the defaults
            std::vector<int> which;
            for (int v = 5; v < 120; v += 2) which.push_back(v);
            g.marginalizeNoOptimize(which, o);
            const spg_marg_stats &st = g.lastStats();
            if (st.n_bad_status != 0 || st.n_removed != (int)which.size()) { std::printf("pass %d: %d bad blankets, %d removed\n", pass, st.n_bad_status, st.n_removed); return 5; }
            kld[pass] = g.lastKullbackLeiblerSum();
            edges[pass] = (int)g.edgeRecords().size();
            if (!std::isfinite(kld[pass])) { std::printf("pass %d: kld sum %g\n", pass, kld[pass]); return 6; }
        }
        std::printf("Subgraph(0.5): interior point kld sum %.9g (%d edges), factor descent %.9g (%d edges)\n", kld[0], edges[0], kld[1], edges[1]);
        if (edges[0] != edges[1]) { std::printf("the two solvers leave different numbers of edges\n"); return 7; }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    std::printf("factor descent ok\n");
    return 0;
}
