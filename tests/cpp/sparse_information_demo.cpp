// tests/cpp/sparse_information_demo.cpp — the block-CSR members of the C++ façade (include/spg_graph_wrapper.hpp:
// sparseInformation / informationApply, GraphWrapperG2O::sparseInformation, src/graph_wrapper_g2o.cpp:382-396) and the PCG
// solver selection, driven from C++ (tests/test_sparse_information.py).
//
//   sparse_information_demo <graph.g2o>   exports the matrix, checks H x against the exported blocks, optimises with PCG
//   sparse_information_demo               usage, exit 2
#include <cmath>
#include <cstdio>
#include <vector>

#include "spg_graph_wrapper.hpp"

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: sparse_information_demo <graph.g2o>\n");
        return 2;
    }
    try {
        spg::GraphWrapperHIP g(argv[1]);
        spg::GraphWrapperHIP::BlockCSR H;
        g.sparseInformation(H);
        const int d = H.blockDim, nb = H.rows();
        if ((int)H.rowPtr.size() != nb + 1 || H.rowPtr[nb] != H.blocks() || (int64_t)H.values.size() != H.blocks() * d * d) {
            std::printf("shape mismatch\n");
            return 3;
        }
        // y = H x on the device against the product with the exported blocks
        std::vector<double> x((size_t)nb * d), ref((size_t)nb * d, 0.0);
        for (size_t i = 0; i < x.size(); i++) x[i] = std::sin(0.37 * (double)i) + 0.25;
        for (int i = 0; i < nb; i++)
            for (int64_t k = H.rowPtr[i]; k < H.rowPtr[i + 1]; k++)
                for (int r = 0; r < d; r++)
                    for (int c = 0; c < d; c++) ref[(size_t)i * d + r] += H.values[(size_t)k * d * d + r * d + c] * x[(size_t)H.colIdx[k] * d + c];
        std::vector<double> y = g.informationApply(x);
        double worst = 0, scale = 0;
        for (size_t i = 0; i < y.size(); i++) { worst = std::fmax(worst, std::fabs(y[i] - ref[i])); scale = std::fmax(scale, std::fabs(ref[i])); }
        if (!(worst <= 1e-12 * std::fmax(scale, 1.0))) { std::printf("H x differs from the exported blocks by %g\n", worst); return 4; }
        g.setLinearSolver(spg::GraphWrapperHIP::SolverPCG);
        g.optimize();
        const spg_pcg_stats st = g.pcgStats();
        std::printf("%d block rows, %lld blocks; PCG: %d solves, %lld iterations, %d unconverged\n", nb, (long long)H.blocks(), st.solves,
                    (long long)st.iterations, st.unconverged);
        if (st.solves <= 0) { std::printf("optimize() did not run PCG\n"); return 5; }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    std::printf("sparse information ok\n");
    return 0;
}
