// tests/cpp/compat_demo.cpp — joint compatibility of candidates through the C++ façade (include/spg_graph_wrapper.hpp:
// compatibleCandidates, include/spg.h: spg_graph_compatible_candidates), tests/test_candidate_compatibility.py.
//
//   compat_demo <graph.g2o> <k> <pair_max_d2> <out.txt>   candidates: the pairs (v_i, v_{n-1-i}) for i < n / 2 (ascending id
//                                           order) with the information of the first edge at v_0; the first half measured
//                                           at their own current relative pose (mutually consistent), the rest at the
//                                           relative pose of the NEXT pair; no individual gate, no joint gate; writes
//                                           "index joint_d2" per accepted candidate, in order
//   compat_demo                             usage, exit 2
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "spg_graph_wrapper.hpp"

int main(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: compat_demo <graph.g2o> <k> <pair_max_d2> <out.txt>\n");
        return 2;
    }
    try {
        spg::GraphWrapperHIP g(argv[1]);
        const int k = std::atoi(argv[2]);
        const double pair_max = std::atof(argv[3]);
        std::vector<int> ids;
        for (const spg::GraphWrapper::Vertex *v : g.vertices()) ids.push_back(v->id());
        const int n = (int)ids.size();
        std::vector<std::pair<int, int>> pairs;
        for (int i = 0; i < n / 2; i++) pairs.push_back({ids[i], ids[n - 1 - i]});
        std::vector<std::pair<spg::VectorXd, spg::MatrixXd>> R = g.relativeCovariances(pairs);
        const spg::MatrixXd info = g.vertices().at(0)->edges().at(0)->information();
        std::vector<spg::GraphWrapperHIP::Candidate> cands;
        for (size_t i = 0; i < pairs.size(); i++)
            cands.push_back({pairs[i].first, pairs[i].second, R[i < pairs.size() / 2 ? i : (i + 1) % pairs.size()].first, info});
        spg_compat_stats st;
        spg::GraphWrapperHIP::CompatResult C = g.compatibleCandidates(cands, k, 0.0, pair_max, {}, -1, &st);
        FILE *f = std::fopen(argv[4], "w");
        if (!f) return 4;
        for (size_t t = 0; t < C.compatible.size(); t++) std::fprintf(f, "%d %.17g\n", C.compatible[t], C.joint_d2[t]);
        std::fclose(f);
        int marked = 0;
        for (int s : C.status) marked += s == SPG_CAND_SELECTED;
        if (marked != (int)C.compatible.size() || st.clique_size != (int)C.clique.size()) {
            std::printf("status and clique size disagree with the result\n");
            return 3;
        }
        bool threw = false;
        try {
            g.compatibleCandidates(cands, k, 0.0, 0.0);   // pair_max_d2 <= 0: SPG_EINVAL, reported as an exception
        } catch (const std::exception &) {
            threw = true;
        }
        std::printf("%zu of %zu candidates accepted, consistent set of %d (seed %d), %lld consistent pairs over %d endpoints; pairs %.2f ms, set %.2f ms, "
                    "gate %.2f ms\n", C.compatible.size(), cands.size(), st.clique_size, st.seed, (long long)st.consistent_pairs, st.endpoints,
                    st.pair_seconds * 1e3, st.clique_seconds * 1e3, st.verify_seconds * 1e3);
        if (!threw) { std::printf("pair_max_d2 = 0 was accepted\n"); return 5; }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    std::printf("compatibility ok\n");
    return 0;
}
