// csrc/spg_greedy_plan.hpp — the column cache of the lazy greedy selection / pruning: which endpoint
// vertices get their D columns of Sigma solved in a round's panel, which cache strip each lands in, and what is evicted.
//
// A round conditions every candidate on the chosen one, i*, and reads only the columns of Sigma at its two endpoints.
// Columns belong to the ORIGINAL Sigma, so a strip never goes stale during a call and any column may be solved ahead of
// time: the rest of the panel is padded with the endpoints of the next-best candidates (speculation). Vertices are named
// by their slot in the endpoint set S; -1 is the fixed vertex, whose blocks are zero: it never gets a strip.
//
// Plain C++: no HIP call and no allocation beyond its own vectors, so the rules can be exercised without a device
// (tests/cpp/lazy_greedy_plan_demo.cpp). The driver (spg_sparse.inc: greedy_lazy_rounds) runs plan() once per round.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace spg {

constexpr int kGreedyPanel = 64;   // scalar width of one right-hand-side panel of the per-round sweeps

// lookahead as the interface takes it -> candidates whose endpoint columns one panel may hold (0 = a full panel)
inline int greedy_lookahead(int requested, int D) {
    const int cap = std::max(1, kGreedyPanel / (2 * D));
    return requested <= 0 ? cap : std::min(requested, cap);
}

struct GreedyRound {
    std::vector<int32_t> solve_vertex, solve_strip;   // columns to solve this round and the strip each lands in
    std::vector<int32_t> evicted;                     // vertices whose strips were given up to make room
    int32_t strip_a = -1, strip_b = -1;               // strips of the chosen candidate's endpoints (-1: the fixed vertex)
    int32_t hits = 0;                                 // endpoint columns of the chosen candidate already cached
    int32_t speculative = 0;                          // of solve_vertex: solved ahead for the next-best candidates
};

class GreedyColumnCache {
public:
    // m endpoint vertices, `strips` cache strips (at least 2: one round needs two), panel_vertices = columns vertices one
    // panel holds (kGreedyPanel / D), lookahead = candidates per panel as greedy_lookahead returns it
    GreedyColumnCache(int m, int strips, int panel_vertices, int lookahead)
        : strip_of_((size_t)m, -1), nstrips_(std::max(2, strips)), panel_(std::max(2, panel_vertices)), lookahead_(std::max(1, lookahead)) {
        vertex_.reserve((size_t)nstrips_);
    }
    int strips() const { return nstrips_; }
    int used_strips() const { return (int)vertex_.size(); }
    int strip_of(int32_t v) const { return v < 0 ? -1 : strip_of_[(size_t)v]; }
    int64_t column_vertices = 0, column_hits = 0, evictions = 0;

    // ranked[0] = i*, ranked[1..] = the next-best eligible candidates in order (-1 ends the list); sa / sb = the endpoint
    // slots per candidate. Needed columns come first; speculation fills what is left of a panel that has a needed column
    // in it, while free strips last, and never evicts. A needed column without a free strip replaces the oldest speculative strip that was never used,
    // else the oldest strip this round does not read.
    void plan(const int32_t *ranked, int nranked, const int32_t *sa, const int32_t *sb, GreedyRound &out) {
        out.solve_vertex.clear(); out.solve_strip.clear(); out.evicted.clear();
        out.hits = 0; out.speculative = 0;
        const int32_t need[2] = {sa[ranked[0]], sb[ranked[0]]};
        for (int e = 0; e < 2; e++) {   // what is cached is marked used before anything is evicted
            const int32_t v = need[e];
            if (v < 0 || (e == 1 && v == need[0])) continue;
            const int s = strip_of_[(size_t)v];
            if (s >= 0) { out.hits++; column_hits++; used_[(size_t)s] = 1; }
        }
        for (int e = 0; e < 2; e++) {
            const int32_t v = need[e];
            if (v < 0 || strip_of_[(size_t)v] >= 0) continue;
            int s = -1;
            if ((int)vertex_.size() < nstrips_) {
                s = (int)vertex_.size();
                vertex_.push_back(-1); used_.push_back(0); age_.push_back(0);
            } else {
                s = victim(need[0], need[1]);
                out.evicted.push_back(vertex_[(size_t)s]);
                strip_of_[(size_t)vertex_[(size_t)s]] = -1;
                evictions++;
            }
            place(v, s, 1, out);
        }
        // a round whose columns are all cached sweeps nothing: speculation rides on a panel that is needed anyway
        const int nlook = out.solve_vertex.empty() ? 0 : std::min(nranked, lookahead_);
        for (int r = 1; r < nlook && ranked[r] >= 0; r++) {
            const int32_t ends[2] = {sa[ranked[r]], sb[ranked[r]]};
            for (int e = 0; e < 2; e++) {
                const int32_t v = ends[e];
                if (v < 0 || strip_of_[(size_t)v] >= 0) continue;
                if ((int)out.solve_vertex.size() >= panel_ || (int)vertex_.size() >= nstrips_) goto done;
                vertex_.push_back(-1); used_.push_back(0); age_.push_back(0);
                place(v, (int)vertex_.size() - 1, 0, out);
                out.speculative++;
            }
        }
    done:
        out.strip_a = strip_of(need[0]);
        out.strip_b = strip_of(need[1]);
        column_vertices += (int64_t)out.solve_vertex.size();
    }

private:
    std::vector<int32_t> strip_of_;   // per endpoint vertex: its strip or -1
    std::vector<int32_t> vertex_;     // per strip: its vertex
    std::vector<uint8_t> used_;       // per strip: a chosen candidate has read it
    std::vector<int64_t> age_;        // per strip: when it was filled
    int nstrips_, panel_, lookahead_;
    int64_t clock_ = 0;

    void place(int32_t v, int s, int used, GreedyRound &out) {
        vertex_[(size_t)s] = v; used_[(size_t)s] = (uint8_t)used; age_[(size_t)s] = ++clock_;
        strip_of_[(size_t)v] = s;
        out.solve_vertex.push_back(v);
        out.solve_strip.push_back(s);
    }
    int victim(int32_t keep_a, int32_t keep_b) const {
        int best = -1;
        for (int pass = 0; pass < 2 && best < 0; pass++)
            for (int s = 0; s < (int)vertex_.size(); s++) {
                if (vertex_[(size_t)s] == keep_a || vertex_[(size_t)s] == keep_b) continue;
                if (pass == 0 && used_[(size_t)s]) continue;
                if (best < 0 || age_[(size_t)s] < age_[(size_t)best]) best = s;
            }
        return best;   // >= 0: at least two strips exist and at most one of them is kept
    }
};

}  // namespace spg
