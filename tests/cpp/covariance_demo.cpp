// tests/cpp/covariance_demo.cpp — the per-pose covariance members of the C++ façade (include/spg_graph_wrapper.hpp:
// marginalCovariances / jointCovariances / marginalKullbackLeibler, what GraphWrapperISAM::covariance reads from iSAM's
// factor, src/graph_wrapper_isam.cpp:259-262) driven from C++ (tests/test_covariance_blocks.py).
//
//   covariance_demo <graph.g2o> <out.txt>   baseline = the file; sparsified = the file after NFR Tree (Global linearisation
//                                           point) of the odd vertices from 5 on; writes, one value per line: every marginal
//                                           block of the sparsified graph (ascending id), the joint block of every vertex
//                                           pair of its edges (sorted), the per-vertex KLD against the baseline
//   covariance_demo                         usage, exit 2
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "spg_graph_wrapper.hpp"

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: covariance_demo <graph.g2o> <out.txt>\n");
        return 2;
    }
    try {
        spg::GraphWrapperHIP base(argv[1]), sp(argv[1]);
        const int nv = (int)sp.vertices().size();
        std::vector<int> which;
        for (int i = 4; i < nv; i++) if (i % 2) which.push_back(sp.vertices()[i]->id());
        spg::SparsityOptions o;
        o.linPoint = spg::SparsityOptions::Global;
        sp.marginalizeNoOptimize(which, o);
        spg_cov_stats st;
        std::vector<spg::MatrixXd> M = sp.marginalCovariances({}, -1, &st);
        std::set<std::pair<int, int>> pr;
        for (const spg::GraphWrapper::Vertex *v : sp.vertices())
            for (const spg::GraphWrapper::Edge *e : v->edges()) {
                std::vector<const spg::GraphWrapper::Vertex *> vs = e->vertices();
                for (size_t a = 0; a < vs.size(); a++)
                    for (size_t b = a + 1; b < vs.size(); b++) pr.insert({vs[a]->id(), vs[b]->id()});
            }
        std::vector<std::pair<int, int>> pairs(pr.begin(), pr.end());
        std::vector<spg::MatrixXd> J = sp.jointCovariances(pairs);
        std::vector<int> ids;
        std::vector<double> kld = base.marginalKullbackLeibler(&sp, &ids);
        if ((int)M.size() != (int)sp.vertices().size() || (int)ids.size() + 1 != (int)M.size() || M[0].rows() != 6 || J[0].rows() != 12) {
            std::printf("shape mismatch\n");
            return 3;
        }
        FILE *f = std::fopen(argv[2], "w");
        if (!f) return 4;
        for (const spg::MatrixXd &m : M) for (double x : m.storage()) std::fprintf(f, "%.17g\n", x);
        for (const spg::MatrixXd &m : J) for (double x : m.storage()) std::fprintf(f, "%.17g\n", x);
        for (double x : kld) std::fprintf(f, "%.17g\n", x);
        std::fclose(f);
        bool threw = false;
        try {
            sp.jointCovariances({{ids[0], ids.back()}});   // no common edge: SPG_EINVAL, reported as an exception
        } catch (const std::exception &) {
            threw = true;
        }
        std::printf("%zu marginal, %zu joint blocks, %zu KLDs, %d supernodes, %.2f ms\n", M.size(), J.size(), kld.size(), st.supernodes,
                    st.device_seconds * 1e3);
        if (!threw) { std::printf("a pair without a common edge was accepted\n"); return 5; }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    std::printf("covariance ok\n");
    return 0;
}
