// The round planner (csrc/spg_round_plan.hpp) under SPG_FLAG_NFR_FACTOR_DESCENT, on hand-built round descriptors and
// without a device (tests/test_factor_descent.py): the Newton-system limit of the interior point does not apply to a
// flagged round, its workspace holds no Hessian, and nothing else about a plan changes.
// Links libspg_hip.so for nfr_ip_pattern_size / nfr_ip_workspace / nfr_fd_workspace only.
#include <cstdio>
#include <cstring>
#include <vector>
#include "spg_round_plan.hpp"

using namespace spg;

namespace {

int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

// blankets with one removed vertex (local index 0) and k kept ones, a pose-pose edge from the removed vertex to each
struct Round {
    spg_options o{};
    std::vector<spg_blanket_desc> bl;
    std::vector<int64_t> vpo;
    std::vector<spg_edge_ref> er;
    std::vector<int32_t> ev;
    spg_round_desc rd{};
    Round(int D, int topo, int flags, double chord = 1.0) {
        o.pose_dim = D; o.algorithm = SPG_ALG_NFR; o.topology = topo; o.lin_point = SPG_LIN_GLOBAL; o.include_intra_clique = 1; o.flags = flags; o.chord_ratio = chord;
    }
    Round &add(int k) {
        spg_blanket_desc bd{};
        bd.vert_begin = (int32_t)vpo.size(); bd.n_vert = k + 1; bd.n_remove = 1;
        bd.edge_begin = (int32_t)er.size(); bd.n_edge = k;
        bd.n_new_max = k * (k - 1) / 2 + 1; bd.n_new_vert_max = 2 * bd.n_new_max; bd.pad_ = 0;
        bd.new_off = 0; bd.new_len = 0; bd.out_off = 64 * (int64_t)bl.size(); bd.tinfo_off = -1;
        for (int v = 0; v <= k; v++) vpo.push_back(0);
        for (int v = 1; v <= k; v++) {
            spg_edge_ref r{};
            r.off = 0; r.len = o.pose_dim == 6 ? 28 : 9; r.kind = SPG_EDGE_BINARY; r.vbegin = (int32_t)ev.size(); r.nv = 2;
            ev.push_back(0); ev.push_back(v);
            er.push_back(r);
        }
        bl.push_back(bd);
        return *this;
    }
    const spg_round_desc *desc() {
        rd.opts = &o; rd.n_blankets = rd.count = (int32_t)bl.size(); rd.first = 0;
        rd.blankets = bl.data(); rd.vert_pose_off = vpo.data(); rd.edges = er.data(); rd.edge_vert = ev.data();
        rd.n_vert_total = (int64_t)vpo.size(); rd.n_edge_total = (int64_t)er.size(); rd.n_edge_vert_total = (int64_t)ev.size();
        rd.mail_base = 0; rd.mail_len = 64 * (int64_t)bl.size(); rd.slot = 0; rd.tag = 1;
        return &rd;
    }
};

struct Planned { RoundPlan P; int rc = 0; char err[512] = {0}; };
void plan(Round &r, const WorkerState &ws, Planned &out) {
    PlanConfig c;
    c.lds_limit = 160 * 1024; c.large_bar = true; c.worker_enabled = true;
    out.rc = plan_round(r.desc(), c, ws, out.P, out.err, sizeof out.err);
}
const WorkerState kNoWorker{1, 0, false}, kWorkerRunning{3, 0, true};

bool same_plan(const RoundPlan &a, const RoundPlan &b) {
    bool same = a.to_worker == b.to_worker && a.cooldown == b.cooldown && a.ip_list == b.ip_list && a.ip_closed == b.ip_closed &&
                a.ip_stride == b.ip_stride && a.ip_hot == b.ip_hot && a.big_list == b.big_list;
    for (int i = 0; i < kPlanBins; i++) {
        const PlanBin &x = a.bins[i], &y = b.bins[i];
        same = same && x.list == y.list && x.kmax == y.kmax && x.mmax == y.mmax && x.lds == y.lds && x.gws_stride == y.gws_stride &&
               x.variant.NT == y.variant.NT && x.variant.gws == y.variant.gws && x.variant.alg == y.variant.alg;
    }
    return same;
}

}  // namespace

int main() {
    const int F = SPG_FLAG_NFR_FACTOR_DESCENT;
    CHECK(F == 8);
    {   // 23 kept SE3 poses under Dense: 253 new edges, a 9 108-variable Newton system — beyond the interior point
        const int k = 23, E = nfr_ip_pattern_size(SPG_TOPO_DENSE, 1.0, k);
        CHECK(E == 253 && 36 * E == 9108 && 36 * E > kIpMaxVars);
        Round plain(6, SPG_TOPO_DENSE, 0);
        plain.add(k);
        Planned pe;
        plan(plain, kNoWorker, pe);
        CHECK(pe.rc == SPG_ECAPACITY);
        char want[512];
        snprintf(want, sizeof want, "interior-point / correlated NFR: a blanket with k=%d kept vertices and %d new measurements is beyond the generic kernel (Newton systems up to %d variables; k <= 64 for CliqueySubgraph, 256 otherwise)", k, E, kIpMaxVars);
        CHECK(strcmp(pe.err, want) == 0);
        // flagged: planned, a workspace without the Hessian — smaller than what an unflagged 12-pose blanket needs
        Round fd(6, SPG_TOPO_DENSE, F);
        fd.add(k).add(2);
        Planned pf;
        plan(fd, kNoWorker, pf);
        CHECK(pf.rc == 0 && !pf.P.to_worker);
        CHECK(pf.P.ip_list == std::vector<int32_t>{0} && pf.P.ip_closed == 0);
        int64_t hot = 0, hot12 = 0;
        const int64_t ws = nfr_fd_workspace(6, k, 1, E, &hot), ws12 = nfr_ip_workspace(6, 12, 1, 66, 0, &hot12);
        CHECK(pf.P.ip_stride == ws && pf.P.ip_hot == hot);
        CHECK(ws < ws12);
        CHECK(ws12 > (int64_t)2376 * 2376);        // the unflagged one holds the (d^2 E)^2 Hessian,
        CHECK(ws < (int64_t)9108 * 9108 / 64);     // the flagged one nothing of that order
        printf("k=23 SE3 Dense: flagged workspace %lld doubles (hot %lld); unflagged k=12: %lld\n", (long long)ws, (long long)hot, (long long)ws12);
    }
    {   // the generic kernel's own limit stays: k <= 256
        Round r(3, SPG_TOPO_DENSE, F);
        r.add(257);
        Planned p;
        plan(r, kNoWorker, p);
        CHECK(p.rc == SPG_ECAPACITY);
        Round ok(3, SPG_TOPO_DENSE, F);
        ok.add(44);      // 43 SE2 poses are the interior point's last size; 44: 8 514 variables
        Planned q, q0;
        plan(ok, kNoWorker, q);
        CHECK(q.rc == 0 && q.P.ip_list == std::vector<int32_t>{0});
        Round no(3, SPG_TOPO_DENSE, 0);
        no.add(44);
        plan(no, kNoWorker, q0);
        CHECK(q0.rc == SPG_ECAPACITY);
    }
    {   // a tree-shaped Subgraph blanket is no interior-point blanket: flagged or not, the same plan; the one with a chord
        // takes the factor-descent workspace
        Round a(6, SPG_TOPO_SUBGRAPH, 0, 0.34), b(6, SPG_TOPO_SUBGRAPH, F, 0.34);
        a.add(3).add(2);                         // (1.34 * 2) = 2 edges for k = 3: a tree
        b.add(3).add(2);
        Planned pa, pb;
        plan(a, kNoWorker, pa); plan(b, kNoWorker, pb);
        CHECK(pa.rc == 0 && pb.rc == 0 && pa.P.ip_list.empty() && same_plan(pa.P, pb.P));
        Round c(6, SPG_TOPO_SUBGRAPH, F, 0.34);
        c.add(4);                                // (1.34 * 3) = 4 edges for k = 4
        Planned pc;
        plan(c, kNoWorker, pc);
        int64_t hot = 0;
        CHECK(pc.rc == 0 && pc.P.ip_list == std::vector<int32_t>{0} && pc.P.ip_closed == 0);
        CHECK(pc.P.ip_stride == nfr_fd_workspace(6, 4, 1, 4, &hot) && pc.P.ip_hot == hot);
    }
    {   // patterns the flag does not apply to: the plan of a flagged round is the plan of the unflagged one — Tree rounds
        // still go to the persistent worker, correlated patterns keep the closed-form workspace
        for (int topo : {SPG_TOPO_TREE, SPG_TOPO_CLIQUEY_SUBGRAPH, SPG_TOPO_CLIQUEY_DENSE}) {
            for (const WorkerState &ws : {kNoWorker, kWorkerRunning}) {
                Round a(6, topo, 0), b(6, topo, F);
                a.add(3).add(5).add(2);
                b.add(3).add(5).add(2);
                Planned pa, pb;
                plan(a, ws, pa); plan(b, ws, pb);
                CHECK(pa.rc == 0 && pb.rc == 0 && same_plan(pa.P, pb.P));
                if (topo == SPG_TOPO_TREE && ws.running) CHECK(pa.P.to_worker && pb.P.to_worker);
            }
        }
    }
    if (failures) { printf("%d FAILED\n", failures); return 1; }
    printf("factor descent plan ok\n");
    return 0;
}
