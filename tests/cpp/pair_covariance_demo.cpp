// tests/cpp/pair_covariance_demo.cpp — the pair / set covariance members of the C++ façade (include/spg_graph_wrapper.hpp:
// pairCovariances / jointMarginalCovariance, iSAM's covariances().marginal(list) as GraphWrapperISAM::covariance asks for
// it, src/graph_wrapper_isam.cpp:259-262) driven from C++ (tests/test_pair_covariances.py).
//
//   pair_covariance_demo <graph.g2o> <out.txt>   writes, one value per line: the pair blocks of (v_0, v_i) for every other
//                                                vertex v_i and of (v_i, v_{n-1-i}) for i < n / 2 (ascending id order), then
//                                                the joint marginal covariance of every 7th vertex
//   pair_covariance_demo                         usage, exit 2
#include <cstdio>
#include <utility>
#include <vector>

#include "spg_graph_wrapper.hpp"

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: pair_covariance_demo <graph.g2o> <out.txt>\n");
        return 2;
    }
    try {
        spg::GraphWrapperHIP g(argv[1]);
        std::vector<int> ids;
        for (const spg::GraphWrapper::Vertex *v : g.vertices()) ids.push_back(v->id());
        const int n = (int)ids.size();
        std::vector<std::pair<int, int>> pairs;
        for (int i = 1; i < n; i++) pairs.push_back({ids[0], ids[i]});
        for (int i = 0; i < n / 2; i++) pairs.push_back({ids[i], ids[n - 1 - i]});
        spg_cov_solve_stats st;
        std::vector<spg::MatrixXd> P = g.pairCovariances(pairs, -1, &st);
        std::vector<int> set;
        for (int i = 0; i < n; i += 7) set.push_back(ids[i]);
        spg::MatrixXd S = g.jointMarginalCovariance(set);
        const int d = (int)P[0].rows() / 2;
        if ((int)P.size() != (int)pairs.size() || S.rows() != (int)set.size() * d) {
            std::printf("shape mismatch\n");
            return 3;
        }
        FILE *f = std::fopen(argv[2], "w");
        if (!f) return 4;
        for (const spg::MatrixXd &m : P) for (double x : m.storage()) std::fprintf(f, "%.17g\n", x);
        for (double x : S.storage()) std::fprintf(f, "%.17g\n", x);
        std::fclose(f);
        bool threw = false;
        try {
            g.pairCovariances({{ids[1], ids[1]}});   // a == b: SPG_EINVAL, reported as an exception
        } catch (const std::exception &) {
            threw = true;
        }
        std::printf("%zu pair blocks, a %d x %d joint marginal; %d columns in %d batches, %.2f ms (solves %.2f ms)\n", P.size(), (int)S.rows(),
                    (int)S.rows(), st.columns, st.rhs_batches, st.cov.device_seconds * 1e3, st.solve_seconds * 1e3);
        if (!threw) { std::printf("a pair (a, a) was accepted\n"); return 5; }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    std::printf("pair covariance ok\n");
    return 0;
}
