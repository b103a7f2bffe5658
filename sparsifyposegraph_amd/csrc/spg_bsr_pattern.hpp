// csrc/spg_bsr_pattern.hpp — block-CSR pattern of a graph's Gauss-Newton information (host only, no HIP):
// the symbolic half of spg_graph_sparse_information / _information_apply and of the PCG solver (spg_bsr.inc).
//
// Block rows and columns are the variables of a staged graph (DenseGraphIn: pos >= 0), numbered by ascending pos.
// The pattern is the full symmetric one — both triangles, columns ascending within a row, the diagonal block always
// present — from all three edge kinds: a binary edge gives its pair, a GLC or MULTI edge the clique of its q vertices.
// A self-loop and an endpoint that is not a variable (the fixed vertex) contribute nothing; parallel edges share a block.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/spg.h"

namespace spg {
namespace bsr {

struct Pattern {
    int nb = 0;                       // block rows
    std::vector<int64_t> row_ptr;     // nb + 1
    std::vector<int32_t> col;         // nnzb block columns, ascending within a row
    std::vector<int64_t> diag;        // nb: index of block (i, i)
    int64_t nnzb() const { return (int64_t)col.size(); }
};

// pos[v]: step * block number of vertex v (step = 1: block numbers, step = D: scalar offsets), -1 = not a variable
inline void build_pattern(int nv, const int32_t *pos, int step, int ne, const spg_edge_ref *er, const int32_t *ev, Pattern &out) {
    int nb = 0;
    for (int v = 0; v < nv; v++) if (pos[v] >= 0) nb++;
    std::vector<uint64_t> key;        // (row << 32) | column
    key.reserve((size_t)nb + 4 * (size_t)ne);
    for (int i = 0; i < nb; i++) key.push_back(((uint64_t)i << 32) | (uint32_t)i);
    for (int e = 0; e < ne; e++) {
        const spg_edge_ref &r = er[e];
        for (int i = 0; i < r.nv; i++) {
            const int32_t pi = pos[ev[r.vbegin + i]];
            if (pi < 0) continue;
            const uint32_t bi = (uint32_t)(pi / step);
            for (int j = i + 1; j < r.nv; j++) {
                const int32_t pj = pos[ev[r.vbegin + j]];
                if (pj < 0 || pj == pi) continue;
                const uint32_t bj = (uint32_t)(pj / step);
                key.push_back(((uint64_t)bi << 32) | bj);
                key.push_back(((uint64_t)bj << 32) | bi);
            }
        }
    }
    std::sort(key.begin(), key.end());
    key.erase(std::unique(key.begin(), key.end()), key.end());
    out.nb = nb;
    out.row_ptr.assign((size_t)nb + 1, 0);
    out.col.resize(key.size());
    out.diag.assign((size_t)nb, 0);
    for (size_t k = 0; k < key.size(); k++) {
        const int32_t i = (int32_t)(key[k] >> 32), j = (int32_t)(key[k] & 0xffffffffu);
        out.row_ptr[(size_t)i + 1]++;
        out.col[k] = j;
        if (i == j) out.diag[(size_t)i] = (int64_t)k;
    }
    for (int i = 0; i < nb; i++) out.row_ptr[(size_t)i + 1] += out.row_ptr[(size_t)i];
}

}  // namespace bsr
}  // namespace spg
