// The round planner of the HIP backend (csrc/spg_round_plan.hpp) on hand-built round descriptors, without a device:
// for the smallest shapes at which each routing rule flips, where does every blanket go — persistent worker, one of
// the LDS bins (and which kernel variant launches it), the generic interior-point / closed-form kernel, the
// large-blanket pipeline, or SPG_ECAPACITY. The expectations are read off the rules, not off the planner's output.
// Links libspg_hip.so for nfr_ip_pattern_size / nfr_ip_workspace only.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "spg_round_plan.hpp"

using namespace spg;

namespace {

int failures = 0, cases = 0;
std::string current;
#define CHECK(c) do { if (!(c)) { printf("FAIL [%s] %s:%d: %s\n", current.c_str(), __FILE__, __LINE__, #c); failures++; } } while (0)

// A round of blankets with m removed vertices (local indices 0..m-1) and k kept ones: one pose-pose edge from the first
// removed vertex to every other vertex.
struct Round {
    spg_options o{};
    std::vector<spg_blanket_desc> bl;
    std::vector<int64_t> vpo;
    std::vector<spg_edge_ref> er;
    std::vector<int32_t> ev;
    spg_round_desc rd{};
    Round(int D, int alg, int topo, int lin) {
        o.pose_dim = D; o.algorithm = alg; o.topology = topo; o.lin_point = lin; o.include_intra_clique = 1; o.flags = 0; o.chord_ratio = 1.0;
    }
    Round &add(int k, int m = 1, int count = 1, int first_edge_kind = SPG_EDGE_BINARY) {
        for (int c = 0; c < count; c++) {
            spg_blanket_desc bd{};
            bd.vert_begin = (int32_t)vpo.size(); bd.n_vert = k + m; bd.n_remove = m;
            bd.edge_begin = (int32_t)er.size(); bd.n_edge = k + m - 1;
            bd.n_new_max = k > 0 ? k : 1; bd.n_new_vert_max = 2 * bd.n_new_max; bd.pad_ = 0;
            bd.new_off = 0; bd.new_len = 0; bd.out_off = 64 * (int64_t)bl.size(); bd.tinfo_off = -1;
            for (int v = 0; v < k + m; v++) vpo.push_back(0);
            for (int v = 1; v < k + m; v++) {
                spg_edge_ref r{};
                r.off = 0; r.len = o.pose_dim == 6 ? 28 : 9; r.kind = v == 1 ? first_edge_kind : SPG_EDGE_BINARY; r.vbegin = (int32_t)ev.size(); r.nv = 2;
                ev.push_back(0); ev.push_back(v);
                er.push_back(r);
            }
            bl.push_back(bd);
        }
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

PlanConfig config() {
    PlanConfig c;
    c.lds_limit = 160 * 1024; c.force_one_wave = false; c.large_bar = true; c.worker_enabled = true; c.force_big = false; c.profiling = false;
    return c;
}
const WorkerState kNoWorker{1, 0, false};   // first batch of a call: never a worker batch

struct Planned { RoundPlan P; int rc = 0; char err[512] = {0}; };

// plans the round and checks what holds for every plan: each blanket in exactly one place, lists in round order
void plan(const char *name, Round &r, const PlanConfig &cfg, const WorkerState &ws, Planned &out) {
    current = name; cases++;
    const spg_round_desc *rd = r.desc();
    out.rc = plan_round(rd, cfg, ws, out.P, out.err, sizeof out.err);
    if (out.rc || out.P.to_worker) return;
    std::vector<int> seen(rd->count, 0);
    std::vector<int32_t> want_staged;
    auto ascending = [&](const std::vector<int32_t> &l) { for (size_t i = 1; i < l.size(); i++) if (l[i - 1] >= l[i]) return false; return true; };
    for (const PlanBin &B : out.P.bins) {
        CHECK(ascending(B.list));
        for (int32_t b : B.list) { seen[b]++; want_staged.push_back(b); }
    }
    CHECK(ascending(out.P.ip_list)); CHECK(ascending(out.P.big_list));
    for (int32_t b : out.P.ip_list) { seen[b]++; want_staged.push_back(b); }
    for (int32_t b : out.P.big_list) seen[b]++;
    for (int s : seen) CHECK(s == 1);
    std::vector<int32_t> staged(rd->count, -1);
    const size_t n = staged_list(out.P, staged.data());     // bins 0..4, then the generic list
    staged.resize(n);
    CHECK(staged == want_staged);
    CHECK(out.P.ip_closed <= (int)out.P.ip_list.size());
}

// the bin that holds blanket b (-1: none)
int bin_of(const RoundPlan &P, int32_t b) {
    for (int i = 0; i < kPlanBins; i++) for (int32_t x : P.bins[i].list) if (x == b) return i;
    return -1;
}

// every blanket of the round sits in one bin that is launched by variant (D, nt, gws, alg)
void expect_variant(Round &r, const Planned &pl, int nt, bool gws, int alg) {
    CHECK(pl.rc == 0 && !pl.P.to_worker);
    CHECK(pl.P.ip_list.empty() && pl.P.big_list.empty());
    const int i = bin_of(pl.P, 0);
    CHECK(i >= 0);
    if (i < 0) return;
    const PlanBin &B = pl.P.bins[i];
    CHECK(B.list.size() == r.bl.size());
    CHECK((i == kPlanBins - 1) == gws);
    CHECK(B.variant.D == r.o.pose_dim); CHECK(B.variant.NT == nt); CHECK(B.variant.gws == gws); CHECK(B.variant.alg == alg);
    const int k = r.bl[0].n_vert - r.bl[0].n_remove, m = r.bl[0].n_remove;
    const Layout L = make_layout(r.o.pose_dim, nt, k, m, r.o.algorithm, r.o.topology, 0);
    if (gws) {
        CHECK(B.gws_stride == (((size_t)L.mat_doubles + 31) & ~(size_t)31));
        CHECK(B.lds == (size_t)L.small_doubles * 8);
    } else {
        CHECK(B.lds == (size_t)(L.small_doubles + L.mat_doubles) * 8);   // (these rows stay below lds_limit: no clamp)
        CHECK(B.lds <= 160 * 1024);
    }
}

void variant_row(const char *name, int D, int alg, int topo, int lin, int k, int count, bool one_wave, int nt, bool gws, int kalg) {
    Round r(D, alg, topo, lin);
    r.add(k, 1, count);
    PlanConfig cfg = config();
    cfg.force_one_wave = one_wave;
    Planned pl;
    plan(name, r, cfg, kNoWorker, pl);
    expect_variant(r, pl, nt, gws, kalg);
}

void test_variants() {
    const int G = SPG_LIN_GLOBAL, Lc = SPG_LIN_LOCAL, T = SPG_TOPO_TREE;
    // n = 18 <= kWaveMax: two wavefronts while the launch cannot fill the chip
    variant_row("nfr tree global D6 k3 x1", 6, SPG_ALG_NFR, T, G, 3, 1, false, 128, false, SPG_ALG_NFR);
    variant_row("nfr tree global D6 k3 x512", 6, SPG_ALG_NFR, T, G, 3, 512, false, 128, false, SPG_ALG_NFR);
    variant_row("nfr tree global D6 k3 x513", 6, SPG_ALG_NFR, T, G, 3, 513, false, 64, false, SPG_ALG_NFR);
    variant_row("nfr tree global D6 k3 one wave", 6, SPG_ALG_NFR, T, G, 3, 1, true, 64, false, SPG_ALG_NFR);
    // n = 24 is the last register-resident size, n = 30 > kWaveMax: four wavefronts up to 1024 blankets
    variant_row("nfr tree global D6 k4 x1", 6, SPG_ALG_NFR, T, G, 4, 1, false, 128, false, SPG_ALG_NFR);
    variant_row("nfr tree global D6 k5 x1", 6, SPG_ALG_NFR, T, G, 5, 1, false, 256, false, SPG_ALG_NFR);
    variant_row("nfr tree global D6 k5 x1024", 6, SPG_ALG_NFR, T, G, 5, 1024, false, 256, false, SPG_ALG_NFR);
    variant_row("nfr tree global D6 k5 x1025", 6, SPG_ALG_NFR, T, G, 5, 1025, false, 64, false, SPG_ALG_NFR);
    variant_row("nfr tree global D6 k5 one wave", 6, SPG_ALG_NFR, T, G, 5, 1, true, 64, false, SPG_ALG_NFR);
    // Local linearisation point: the LM variants; no four-wavefront one
    variant_row("nfr tree local D6 k3", 6, SPG_ALG_NFR, T, Lc, 3, 1, false, 128, false, SPG_ALG_NFR_LM);
    variant_row("nfr tree local D6 k5", 6, SPG_ALG_NFR, T, Lc, 5, 1, false, 64, false, SPG_ALG_NFR_LM);
    variant_row("glc tree D6 k3", 6, SPG_ALG_GLC, T, G, 3, 1, false, 64, false, SPG_ALG_GLC);
    // SE2: n = 9
    variant_row("nfr tree global D3 k3 x1", 3, SPG_ALG_NFR, T, G, 3, 1, false, 128, false, SPG_ALG_NFR);
    variant_row("nfr tree global D3 k3 x513", 3, SPG_ALG_NFR, T, G, 3, 513, false, 64, false, SPG_ALG_NFR);
    variant_row("nfr tree global D3 k8 x1", 3, SPG_ALG_NFR, T, G, 8, 1, false, 128, false, SPG_ALG_NFR);
    variant_row("nfr tree global D3 k9 x1", 3, SPG_ALG_NFR, T, G, 9, 1, false, 256, false, SPG_ALG_NFR);
    variant_row("glc tree D3 k3", 3, SPG_ALG_GLC, T, G, 3, 1, false, 64, false, SPG_ALG_GLC);
    // tiles beyond lds_limit (3 x 120 x 121 doubles), side buffers within: the workspace variants
    variant_row("nfr tree global D6 k20", 6, SPG_ALG_NFR, T, G, 20, 1, false, 1024, true, SPG_ALG_NFR);
    variant_row("nfr tree global D6 k20 one wave", 6, SPG_ALG_NFR, T, G, 20, 1, true, 256, true, SPG_ALG_NFR);
    variant_row("nfr tree local D6 k20", 6, SPG_ALG_NFR, T, Lc, 20, 1, false, 256, true, SPG_ALG_NFR_LM);
    variant_row("glc tree D6 k20", 6, SPG_ALG_GLC, T, G, 20, 1, false, 256, true, SPG_ALG_GLC);
}

// smallest k whose side buffers (carve-up of nt lanes) exceed lds_limit
int first_k_beyond(int D, int nt, int alg, int topo, int limit) {
    for (int k = 2; k < 2000; k++) if ((size_t)make_layout(D, nt, k, 1, alg, topo, 0).small_doubles * 8 > (size_t)limit) return k;
    return -1;
}

void test_side_buffers() {
    const PlanConfig cfg = config();
    {   // GLC Dense, Global: the large-blanket pipeline takes over where the side buffers end
        const int kb = first_k_beyond(6, 256, SPG_ALG_GLC, SPG_TOPO_DENSE, cfg.lds_limit);
        CHECK(kb > 2);
        Round r(6, SPG_ALG_GLC, SPG_TOPO_DENSE, SPG_LIN_GLOBAL);
        r.add(kb - 1).add(kb).add(3);
        Planned pl;
        plan("glc dense at the side-buffer limit", r, cfg, kNoWorker, pl);
        CHECK(pl.rc == 0);
        CHECK(bin_of(pl.P, 0) == kPlanBins - 1);
        CHECK(pl.P.big_list == std::vector<int32_t>{1});
        CHECK(bin_of(pl.P, 2) >= 0 && bin_of(pl.P, 2) < kPlanBins - 1);
        const PlanBin &B = pl.P.bins[kPlanBins - 1];
        CHECK(B.kmax == kb - 1);   // the envelope of the bin follows what left it
        CHECK(B.variant.NT == 256 && B.variant.gws && B.variant.alg == SPG_ALG_GLC);
    }
    {   // GLC Tree has no such path
        const int kb = first_k_beyond(6, 256, SPG_ALG_GLC, SPG_TOPO_TREE, cfg.lds_limit);
        Round ok(6, SPG_ALG_GLC, SPG_TOPO_TREE, SPG_LIN_GLOBAL);
        ok.add(kb - 1);
        Planned pl;
        plan("glc tree below the side-buffer limit", ok, cfg, kNoWorker, pl);
        expect_variant(ok, pl, 256, true, SPG_ALG_GLC);
        Round r(6, SPG_ALG_GLC, SPG_TOPO_TREE, SPG_LIN_GLOBAL);
        r.add(kb);
        Planned pe;
        plan("glc tree beyond the side-buffer limit", r, cfg, kNoWorker, pe);
        char want[512];
        snprintf(want, sizeof want, "blanket too large for LDS side buffers: k=%d m=%d (only GLC Dense blankets have a large-blanket path)", kb, 1);
        CHECK(pe.rc == SPG_ECAPACITY);
        CHECK(strcmp(pe.err, want) == 0);
    }
    {   // NFR Tree: the generic kernel's closed form up to k = 256 (only blankets of the LAST bin are tested for it)
        const int kb = first_k_beyond(6, 1024, SPG_ALG_NFR, SPG_TOPO_TREE, cfg.lds_limit);
        CHECK(kb > 2 && kb <= 256);
        Round r(6, SPG_ALG_NFR, SPG_TOPO_TREE, SPG_LIN_GLOBAL);
        r.add(kb - 1).add(kb).add(256).add(3);
        Planned pl;
        plan("nfr tree at the side-buffer limit", r, cfg, kNoWorker, pl);
        CHECK(pl.rc == 0);
        CHECK(bin_of(pl.P, 0) == kPlanBins - 1);
        CHECK((pl.P.ip_list == std::vector<int32_t>{1, 2}));
        CHECK(pl.P.ip_closed == 2);
        CHECK(bin_of(pl.P, 3) >= 0 && bin_of(pl.P, 3) < kPlanBins - 1);
        int64_t hot = 0, hot_kb = 0;   // the workspace slice and its LDS-eligible part: the largest of the list
        const int64_t ws = nfr_ip_workspace(6, 256, 1, 255, 1, &hot), ws_kb = nfr_ip_workspace(6, kb, 1, kb - 1, 1, &hot_kb);
        CHECK(pl.P.ip_stride == (ws > ws_kb ? ws : ws_kb));
        CHECK(pl.P.ip_hot == (hot > hot_kb ? hot : hot_kb));
        CHECK(pl.P.bins[kPlanBins - 1].kmax == kb - 1 && pl.P.bins[kPlanBins - 1].variant.NT == 1024);
        Round r2(6, SPG_ALG_NFR, SPG_TOPO_TREE, SPG_LIN_GLOBAL);
        r2.add(257);
        Planned pe;
        plan("nfr tree k=257", r2, cfg, kNoWorker, pe);
        CHECK(pe.rc == SPG_ECAPACITY);
        char want[512];
        snprintf(want, sizeof want, "interior-point / correlated NFR: a blanket with k=%d kept vertices and %d new measurements is beyond the generic kernel (Newton systems up to %d variables; k <= 64 for CliqueySubgraph, 256 otherwise)", 257, 256, kIpMaxVars);
        CHECK(strcmp(pe.err, want) == 0);
    }
    {   // ... of the last bin: a device limit so low that the 1024-lane side buffers of a blanket exceed it while the
        // blanket as a whole (256-lane carve-up, tiles included) still fits keeps the blanket in its LDS bin
        const Layout L256 = make_layout(3, 256, 2, 1, SPG_ALG_NFR, SPG_TOPO_TREE, 0);
        PlanConfig low = cfg;
        low.lds_limit = (L256.small_doubles + L256.mat_doubles) * 8;
        CHECK((size_t)make_layout(3, 1024, 2, 1, SPG_ALG_NFR, SPG_TOPO_TREE, 0).small_doubles * 8 > (size_t)low.lds_limit);
        Round r(3, SPG_ALG_NFR, SPG_TOPO_TREE, SPG_LIN_GLOBAL);
        r.add(2);
        Planned pl;
        plan("nfr tree D3 k2 at a low device limit", r, low, kNoWorker, pl);
        expect_variant(r, pl, 128, false, SPG_ALG_NFR);
    }
    {   // the Local linearisation point is tested against the 256-lane carve-up
        const int kb = first_k_beyond(6, 256, SPG_ALG_NFR, SPG_TOPO_TREE, cfg.lds_limit);
        Round r(6, SPG_ALG_NFR, SPG_TOPO_TREE, SPG_LIN_LOCAL);
        r.add(kb - 1).add(kb);
        Planned pl;
        plan("nfr tree local at the side-buffer limit", r, cfg, kNoWorker, pl);
        CHECK(pl.rc == 0 && bin_of(pl.P, 0) == kPlanBins - 1 && pl.P.ip_list == std::vector<int32_t>{1});
    }
}

void test_routes() {
    PlanConfig cfg = config();
    {   // SPG_FORCE_BIG: every GLC Dense blanket with two kept vertices and an edge, in ascending order
        cfg.force_big = true;
        Round r(6, SPG_ALG_GLC, SPG_TOPO_DENSE, SPG_LIN_GLOBAL);
        r.add(20).add(2).add(1).add(3).add(20).add(2);
        Planned pl;
        plan("force_big glc dense", r, cfg, kNoWorker, pl);
        CHECK(pl.rc == 0);
        CHECK((pl.P.big_list == std::vector<int32_t>{0, 1, 3, 4, 5}));
        CHECK(bin_of(pl.P, 2) >= 0 && bin_of(pl.P, 2) < kPlanBins - 1);
        Round t(6, SPG_ALG_GLC, SPG_TOPO_TREE, SPG_LIN_GLOBAL);   // ... and nothing else
        t.add(3);
        Planned pt;
        plan("force_big glc tree", t, cfg, kNoWorker, pt);
        expect_variant(t, pt, 64, false, SPG_ALG_GLC);
        cfg.force_big = false;
    }
    {   // NFR Dense: the interior point from three kept vertices on (E = 3 > k - 1)
        Round r(6, SPG_ALG_NFR, SPG_TOPO_DENSE, SPG_LIN_GLOBAL);
        r.add(3).add(2);
        Planned pl;
        plan("nfr dense", r, cfg, kNoWorker, pl);
        CHECK(pl.rc == 0 && pl.P.ip_list == std::vector<int32_t>{0} && pl.P.ip_closed == 0);
        CHECK(bin_of(pl.P, 1) >= 0);
        int64_t hot = 0;
        CHECK(pl.P.ip_stride == nfr_ip_workspace(6, 3, 1, nfr_ip_pattern_size(SPG_TOPO_DENSE, 1.0, 3), 0, &hot) && pl.P.ip_hot == hot);
    }
    {   // correlated patterns: the generic kernel's closed form
        Round r(6, SPG_ALG_NFR, SPG_TOPO_CLIQUEY_DENSE, SPG_LIN_GLOBAL);
        r.add(3).add(2);
        Planned pl;
        plan("nfr cliquey dense", r, cfg, kNoWorker, pl);
        CHECK(pl.rc == 0 && pl.P.ip_list == std::vector<int32_t>{0} && pl.P.ip_closed == 1);
        CHECK(bin_of(pl.P, 1) >= 0);
    }
    {   // a correlated input edge: from two kept vertices on
        Round r(6, SPG_ALG_NFR, SPG_TOPO_TREE, SPG_LIN_GLOBAL);
        r.add(2, 1, 1, SPG_EDGE_MULTI).add(2).add(1, 1, 1, SPG_EDGE_MULTI);
        Planned pl;
        plan("nfr tree with a MULTI edge", r, cfg, kNoWorker, pl);
        CHECK(pl.rc == 0 && pl.P.ip_list == std::vector<int32_t>{0} && pl.P.ip_closed == 1);
        CHECK(bin_of(pl.P, 1) >= 0 && bin_of(pl.P, 2) >= 0);
    }
    {   // CliqueySubgraph fills cliques on 64-bit vertex masks
        Round ok(6, SPG_ALG_NFR, SPG_TOPO_CLIQUEY_SUBGRAPH, SPG_LIN_GLOBAL);
        ok.add(64);
        Planned pl;
        plan("nfr cliquey subgraph k=64", ok, cfg, kNoWorker, pl);
        CHECK(pl.rc == 0 && pl.P.ip_list == std::vector<int32_t>{0} && pl.P.ip_closed == 1);
        Round r(6, SPG_ALG_NFR, SPG_TOPO_CLIQUEY_SUBGRAPH, SPG_LIN_GLOBAL);
        r.add(65);
        Planned pe;
        plan("nfr cliquey subgraph k=65", r, cfg, kNoWorker, pe);
        CHECK(pe.rc == SPG_ECAPACITY && strstr(pe.err, "k=65 kept vertices") != nullptr);
    }
    {   // clusters under the Local linearisation point
        Round r(6, SPG_ALG_NFR, SPG_TOPO_TREE, SPG_LIN_LOCAL);
        r.add(2, 2).add(2, 1).add(1, 2);
        Planned pl;
        plan("nfr tree local cluster", r, cfg, kNoWorker, pl);
        CHECK(pl.rc == 0 && pl.P.ip_list == std::vector<int32_t>{0} && pl.P.ip_closed == 1);
        CHECK(bin_of(pl.P, 1) >= 0 && bin_of(pl.P, 2) >= 0);
        Round g(6, SPG_ALG_NFR, SPG_TOPO_TREE, SPG_LIN_GLOBAL);   // ... only there
        g.add(2, 2);
        Planned pg;
        plan("nfr tree global cluster", g, cfg, kNoWorker, pg);
        CHECK(pg.rc == 0 && pg.P.ip_list.empty() && bin_of(pg.P, 0) >= 0);
    }
}

void test_worker() {
    const PlanConfig cfg = config();
    auto batch = [](int count) { Round r(6, SPG_ALG_NFR, SPG_TOPO_TREE, SPG_LIN_GLOBAL); r.add(3, 1, count); return r; };
    Planned pl;
    {
        Round r = batch(8);
        plan("worker: eligible batch", r, cfg, WorkerState{3, 0, false}, pl);
        CHECK(pl.rc == 0 && pl.P.to_worker && pl.P.cooldown == 0);
    }
    {
        Round r = batch(512);
        plan("worker: 512 blankets", r, cfg, WorkerState{3, 0, false}, pl);
        CHECK(pl.P.to_worker);
        Round r2 = batch(513);
        plan("worker: 513 blankets", r2, cfg, WorkerState{3, 0, false}, pl);
        CHECK(pl.rc == 0 && !pl.P.to_worker && pl.P.cooldown == 0 && bin_of(pl.P, 0) >= 0);
    }
    {
        Round r = batch(4);
        r.add(3, 2);
        plan("worker: one blanket removes two vertices", r, cfg, WorkerState{3, 0, false}, pl);
        CHECK(pl.rc == 0 && !pl.P.to_worker && pl.P.cooldown == 8 && bin_of(pl.P, 4) >= 0);
    }
    {
        Round r = batch(8);
        plan("worker: cool-down 1 on entry", r, cfg, WorkerState{3, 1, false}, pl);
        CHECK(!pl.P.to_worker && pl.P.cooldown == 0);
        plan("worker: cool-down 8 on entry", r, cfg, WorkerState{3, 8, true}, pl);
        CHECK(!pl.P.to_worker && pl.P.cooldown == 7);
    }
    {
        Round r = batch(8);
        plan("worker: second batch of a call, no worker running", r, cfg, WorkerState{2, 0, false}, pl);
        CHECK(!pl.P.to_worker && pl.P.cooldown == 0);
        plan("worker: second batch of a call, worker running", r, cfg, WorkerState{2, 0, true}, pl);
        CHECK(pl.P.to_worker);
    }
    {   // n = 36 is the largest target a worker takes; what the backend cannot offer keeps the launch path
        Round r = batch(2);
        r.add(6);
        plan("worker: k=6", r, cfg, WorkerState{3, 0, false}, pl);
        CHECK(pl.P.to_worker);
        r.add(7);
        plan("worker: k=7", r, cfg, WorkerState{3, 0, false}, pl);
        CHECK(!pl.P.to_worker && pl.P.cooldown == 8);
        Round e = batch(8);
        PlanConfig c2 = cfg; c2.large_bar = false;
        plan("worker: no large BAR", e, c2, WorkerState{3, 0, false}, pl);
        CHECK(!pl.P.to_worker);
        c2 = cfg; c2.worker_enabled = false;
        plan("worker: disabled", e, c2, WorkerState{3, 0, false}, pl);
        CHECK(!pl.P.to_worker);
        c2 = cfg; c2.force_one_wave = true;
        plan("worker: one wave", e, c2, WorkerState{3, 0, false}, pl);
        CHECK(!pl.P.to_worker);
    }
    {   // a plan is rebuilt from scratch each round (the backend keeps one per launch slot)
        Round a(6, SPG_ALG_NFR, SPG_TOPO_DENSE, SPG_LIN_GLOBAL);
        a.add(3).add(20);
        plan("reuse: first round", a, cfg, kNoWorker, pl);
        Round b = batch(2);
        plan("reuse: second round", b, cfg, kNoWorker, pl);
        expect_variant(b, pl, 128, false, SPG_ALG_NFR);
        CHECK(pl.P.ip_stride == 0 && pl.P.ip_hot == 0 && pl.P.ip_closed == 0);
    }
}

}  // namespace

int main() {
    test_variants();
    test_side_buffers();
    test_routes();
    test_worker();
    if (failures) { printf("plan FAILED: %d checks in %d cases\n", failures, cases); return 1; }
    printf("plan ok: %d cases\n", cases);
    return 0;
}
