// tests/cpp/robust_demo.cpp — the robust-kernel members of the C++ façade (include/spg_graph_wrapper.hpp: setRobustKernel /
// robustKernel / edgeChi2, g2o's setRobustKernel on every edge) driven from C++ (tests/test_robust_facade.py).
//
//   robust_demo <graph.g2o>   per-edge chi2 against chi2(), a Cauchy optimize(), the kernel cleared again
//   robust_demo               usage, exit 2
#include <cmath>
#include <cstdio>
#include <vector>

#include "spg_graph_wrapper.hpp"

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: robust_demo <graph.g2o>\n");
        return 2;
    }
    try {
        spg::GraphWrapperHIP g(argv[1]);
        // no kernel: rho = s, w = 1, and the per-edge values sum to chi2()
        spg::GraphWrapperHIP::EdgeChi2 plain = g.edgeChi2();
        double sum = 0;
        for (size_t e = 0; e < plain.chi2.size(); e++) {
            sum += plain.chi2[e];
            if (plain.rho[e] != plain.chi2[e] || plain.weight[e] != 1.0) { std::printf("edge %zu: rho / weight without a kernel\n", e); return 3; }
        }
        const double chi = g.chi2();
        if (!(std::fabs(sum - chi) <= 1e-12 * std::fmax(chi, 1.0))) { std::printf("sum of edge chi2 %.17g != chi2() %.17g\n", sum, chi); return 4; }
        // Cauchy of width 1 on everything but consecutive-id odometry
        g.setRobustKernel(SPG_ROBUST_CAUCHY, 1.0, 2);
        const spg::GraphWrapperHIP::RobustKernel k = g.robustKernel();
        if (k.kind != SPG_ROBUST_CAUCHY || k.delta != 1.0 || k.minIdGap != 2) { std::printf("robustKernel() does not return the setting\n"); return 5; }
        spg::GraphWrapperHIP::EdgeChi2 rob = g.edgeChi2();
        double rho_sum = 0;
        for (size_t e = 0; e < rob.chi2.size(); e++) {
            rho_sum += rob.rho[e];
            if (rob.chi2[e] != plain.chi2[e]) { std::printf("edge %zu: the kernel changed the plain chi2\n", e); return 6; }
            if (!(rob.weight[e] > 0 && rob.weight[e] <= 1.0 && rob.rho[e] <= rob.chi2[e])) { std::printf("edge %zu: weight %g rho %g s %g\n", e, rob.weight[e], rob.rho[e], rob.chi2[e]); return 7; }
        }
        if (g.chi2() != chi) { std::printf("chi2() honours the kernel\n"); return 8; }
        const spg_optimize_stats st = g.optimizeFromId(-1);
        if (!(std::fabs(st.chi2_initial - rho_sum) <= 1e-12 * std::fmax(rho_sum, 1.0))) { std::printf("chi2_initial %.17g != sum rho %.17g\n", st.chi2_initial, rho_sum); return 9; }
        if (!(st.chi2_final <= st.chi2_initial)) { std::printf("the robust cost went up: %g -> %g\n", st.chi2_initial, st.chi2_final); return 10; }
        std::printf("%zu edges; chi2 %.9g, Cauchy cost %.9g -> %.9g in %d iterations\n", rob.chi2.size(), chi, st.chi2_initial, st.chi2_final, st.iterations);
        g.setRobustKernel(SPG_ROBUST_NONE);
        if (g.robustKernel().kind != SPG_ROBUST_NONE) { std::printf("the kernel was not cleared\n"); return 11; }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    std::printf("robust ok\n");
    return 0;
}
