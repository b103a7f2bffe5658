// The column-cache planner of the lazy greedy calls (csrc/spg_greedy_plan.hpp) on scripted ranked lists: no device.
// Prints "ok" and returns 0, or names the first expectation that fails. Built once plainly and once with
// -fsanitize=address,undefined by tests/test_lazy_greedy.py.
#include <cstdio>
#include <set>
#include <vector>
#include "spg_greedy_plan.hpp"

using spg::GreedyColumnCache;
using spg::GreedyRound;

static int fails = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } \
    } while (0)

static bool same(const std::vector<int32_t> &a, std::initializer_list<int32_t> b) { return a == std::vector<int32_t>(b); }

int main() {
    EXPECT(spg::greedy_lookahead(0, 6) == 5 && spg::greedy_lookahead(0, 3) == 10);
    EXPECT(spg::greedy_lookahead(1, 6) == 1 && spg::greedy_lookahead(99, 6) == 5 && spg::greedy_lookahead(7, 3) == 7);
    // candidates: endpoint slots (sa, sb); -1 = the fixed vertex
    const int32_t sa[] = {0, 2, 4, -1, 0, 6, 8}, sb[] = {1, 3, 5, 2, 3, 7, 9};
    {   // a roomy cache, SE3 panel (10 column vertices), lookahead 3
        GreedyColumnCache c(10, 10, 10, 3);
        GreedyRound r;
        const int32_t r0[] = {1, 0, 3, 2};   // chosen 1 = (2, 3); ahead: 0 = (0, 1), 3 = (fixed, 2); 2 is beyond the lookahead
        c.plan(r0, 4, sa, sb, r);
        EXPECT(same(r.solve_vertex, {2, 3, 0, 1}) && same(r.solve_strip, {0, 1, 2, 3}));
        EXPECT(r.strip_a == 0 && r.strip_b == 1 && r.hits == 0 && r.speculative == 2 && r.evicted.empty());
        const int32_t r1[] = {0, 4, -1};     // chosen 0 = (0, 1): both solved ahead; 4 = (0, 3): nothing new; the list ends
        c.plan(r1, 3, sa, sb, r);
        EXPECT(r.solve_vertex.empty() && r.hits == 2 && r.strip_a == 2 && r.strip_b == 3);
        const int32_t r2[] = {3, 2, 5};      // chosen 3 = (fixed, 2): the fixed endpoint has no strip; 2 is cached, so no panel
        c.plan(r2, 3, sa, sb, r);            // is swept and nothing is solved ahead either
        EXPECT(r.strip_a == -1 && r.strip_b == 0 && r.hits == 1);
        EXPECT(r.solve_vertex.empty() && r.speculative == 0);
        const int32_t r3[] = {6, 5, 2};      // chosen 6 = (8, 9): needed, and 5 = (6, 7), 2 = (4, 5) ride along
        c.plan(r3, 3, sa, sb, r);
        EXPECT(same(r.solve_vertex, {8, 9, 6, 7, 4, 5}) && same(r.solve_strip, {4, 5, 6, 7, 8, 9}) && r.speculative == 4);
        EXPECT(r.evicted.empty() && c.used_strips() == 10);
        EXPECT(c.column_vertices == 10 && c.column_hits == 3 && c.evictions == 0);
        EXPECT(c.strip_of(-1) == -1);
    }
    {   // the budget runs out: speculation stops, a needed column replaces the oldest speculative strip never used
        GreedyColumnCache c(10, 4, 10, 3);
        GreedyRound r;
        const int32_t r0[] = {1, 0, 2};      // (2, 3) needed, (0, 1) ahead, then the cache is full: (4, 5) is not solved
        c.plan(r0, 3, sa, sb, r);
        EXPECT(same(r.solve_vertex, {2, 3, 0, 1}) && r.speculative == 2 && c.used_strips() == 4);
        const int32_t r1[] = {2, 0, 5};      // (4, 5) needed: evicts vertices 0 and 1, the speculative strips, oldest first
        c.plan(r1, 3, sa, sb, r);
        EXPECT(same(r.solve_vertex, {4, 5}) && same(r.solve_strip, {2, 3}) && same(r.evicted, {0, 1}) && r.speculative == 0);
        EXPECT(r.strip_a == 2 && r.strip_b == 3 && c.strip_of(0) == -1 && c.strip_of(2) == 0);
        const int32_t r2[] = {0, -1};        // (0, 1) after all: every strip has been used, the oldest not read now goes
        c.plan(r2, 2, sa, sb, r);
        EXPECT(same(r.solve_vertex, {0, 1}) && same(r.evicted, {2, 3}) && same(r.solve_strip, {0, 1}) && c.evictions == 4);
    }
    {   // two strips serve every round, whatever the order; fixed endpoints never get a slot
        GreedyColumnCache c(10, 2, 10, 5);
        GreedyRound r;
        const int order[] = {1, 3, 4, 0, 6, 2, 5, 3, 1};
        for (int i : order) {
            const int32_t rk[] = {i, (i + 1) % 7, (i + 2) % 7};
            c.plan(rk, 3, sa, sb, r);
            EXPECT(r.strip_a == (sa[i] < 0 ? -1 : c.strip_of(sa[i])) && r.strip_b == c.strip_of(sb[i]));
            EXPECT((sa[i] < 0 || (r.strip_a >= 0 && r.strip_a < 2)) && r.strip_b >= 0 && r.strip_b < 2 && r.strip_a != r.strip_b);
            EXPECT(r.speculative == 0 || c.used_strips() <= 2);
            std::set<int32_t> strips(r.solve_strip.begin(), r.solve_strip.end());
            EXPECT(strips.size() == r.solve_strip.size());
            for (int32_t v : r.solve_vertex) EXPECT(v >= 0);
            EXPECT((int)r.solve_vertex.size() + r.hits == (sa[i] >= 0) + 1);
        }
        EXPECT(c.used_strips() == 2);
    }
    {   // the panel's width bounds speculation: 2 needed + at most 2 more with a 4-vertex panel
        GreedyColumnCache c(10, 10, 4, 5);
        GreedyRound r;
        const int32_t r0[] = {0, 1, 2, 5, 6};
        c.plan(r0, 5, sa, sb, r);
        EXPECT(same(r.solve_vertex, {0, 1, 2, 3}) && r.speculative == 2);
    }
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
