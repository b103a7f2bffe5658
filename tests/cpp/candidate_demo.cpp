// tests/cpp/candidate_demo.cpp — the relative-covariance and candidate-score members of the C++ façade
// (include/spg_graph_wrapper.hpp: relativeCovariances / scoreCandidates, include/spg.h: spg_graph_relative_covariances /
// spg_graph_score_candidates) driven from C++ (tests/test_relative_covariance.py).
//
//   candidate_demo <graph.g2o> <out.txt>   writes, one value per line: for the pairs (v_0, v_i) of every other vertex v_i and
//                                          (v_i, v_{n-1-i}) for i < n / 2 (ascending id order) the relative pose and its
//                                          covariance; then d2, gain, chi2 and status of the same pairs as candidates, each
//                                          measured at the relative pose of the NEXT pair of the list with the information
//                                          of the first edge at v_0
//   candidate_demo                         usage, exit 2
#include <cstdio>
#include <utility>
#include <vector>

#include "spg_graph_wrapper.hpp"

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: candidate_demo <graph.g2o> <out.txt>\n");
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
        std::vector<std::pair<spg::VectorXd, spg::MatrixXd>> R = g.relativeCovariances(pairs, -1, &st);
        if (R.size() != pairs.size()) {
            std::printf("shape mismatch\n");
            return 3;
        }
        const spg::MatrixXd info = g.vertices().at(0)->edges().at(0)->information();
        std::vector<spg::GraphWrapperHIP::Candidate> cands;
        for (size_t i = 0; i < pairs.size(); i++) cands.push_back({pairs[i].first, pairs[i].second, R[(i + 1) % pairs.size()].first, info});
        std::vector<spg::GraphWrapperHIP::CandidateScore> S = g.scoreCandidates(cands);
        FILE *f = std::fopen(argv[2], "w");
        if (!f) return 4;
        for (const auto &r : R) {
            for (double x : r.first) std::fprintf(f, "%.17g\n", x);
            for (double x : r.second.storage()) std::fprintf(f, "%.17g\n", x);
        }
        for (const auto &s : S) std::fprintf(f, "%.17g\n%.17g\n%.17g\n%d\n", s.d2, s.gain, s.chi2, s.status);
        std::fclose(f);
        bool threw = false;
        try {
            g.relativeCovariances({{ids[1], ids[1]}});   // a == b: SPG_EINVAL, reported as an exception
        } catch (const std::exception &) {
            threw = true;
        }
        std::printf("%zu relative covariances, %zu scores; %d columns in %d batches, %.2f ms (solves %.2f ms)\n", R.size(), S.size(), st.columns,
                    st.rhs_batches, st.cov.device_seconds * 1e3, st.solve_seconds * 1e3);
        if (!threw) { std::printf("a pair (a, a) was accepted\n"); return 5; }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    std::printf("candidates ok\n");
    return 0;
}
