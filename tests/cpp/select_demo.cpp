// tests/cpp/select_demo.cpp — greedy candidate selection through the C++ façade (include/spg_graph_wrapper.hpp:
// selectCandidates, include/spg.h: spg_graph_select_candidates), tests/test_candidate_selection.py.
//
//   select_demo <graph.g2o> <k> <out.txt>   candidates: the pairs (v_i, v_{n-1-i}) for i < n / 2 (ascending id order), each
//                                           measured at the current relative pose of the NEXT pair of the list with the
//                                           information of the first edge at v_0, every pair of the first five listed a
//                                           second time at the end; selects k of them, writes "index gain" per line in
//                                           order of selection and adds the selected edges to the graph
//   select_demo                             usage, exit 2
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "spg_graph_wrapper.hpp"

int main(int argc, char **argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: select_demo <graph.g2o> <k> <out.txt>\n");
        return 2;
    }
    try {
        spg::GraphWrapperHIP g(argv[1]);
        const int k = std::atoi(argv[2]);
        std::vector<int> ids;
        for (const spg::GraphWrapper::Vertex *v : g.vertices()) ids.push_back(v->id());
        const int n = (int)ids.size();
        std::vector<std::pair<int, int>> pairs;
        for (int i = 0; i < n / 2; i++) pairs.push_back({ids[i], ids[n - 1 - i]});
        std::vector<std::pair<spg::VectorXd, spg::MatrixXd>> R = g.relativeCovariances(pairs);
        const spg::MatrixXd info = g.vertices().at(0)->edges().at(0)->information();
        std::vector<spg::GraphWrapperHIP::Candidate> cands;
        for (size_t i = 0; i < pairs.size(); i++) cands.push_back({pairs[i].first, pairs[i].second, R[(i + 1) % pairs.size()].first, info});
        for (size_t i = 0; i < 5 && i < pairs.size(); i++) cands.push_back(cands[i]);
        std::vector<int> status;
        spg_select_stats st;
        std::vector<std::pair<int, double>> S = g.selectCandidates(cands, k, 0.0, 0.0, -1, &status, &st);
        FILE *f = std::fopen(argv[3], "w");
        if (!f) return 4;
        for (const auto &s : S) std::fprintf(f, "%d %.17g\n", s.first, s.second);
        std::fclose(f);
        int marked = 0;
        for (int s : status) marked += s == SPG_CAND_SELECTED;
        if (marked != (int)S.size() || st.rounds != (int)S.size()) { std::printf("status and rounds disagree with the selection\n"); return 3; }
        for (const auto &s : S) {
            const spg::GraphWrapperHIP::Candidate &c = cands[(size_t)s.first];
            g.addEdge(c.from, c.to, spg::IsometryXd(c.measurement), c.information);
        }
        bool threw = false;
        try {
            g.selectCandidates(cands, -1);   // k < 0: SPG_EINVAL, reported as an exception
        } catch (const std::exception &) {
            threw = true;
        }
        std::printf("%zu of %zu candidates selected over %d endpoints in %d rounds, %.2f ms (selection %.2f ms)\n", S.size(), cands.size(), st.endpoints,
                    st.rounds, st.solve.cov.device_seconds * 1e3, st.select_seconds * 1e3);
        if (!threw) { std::printf("k = -1 was accepted\n"); return 5; }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    std::printf("selection ok\n");
    return 0;
}
