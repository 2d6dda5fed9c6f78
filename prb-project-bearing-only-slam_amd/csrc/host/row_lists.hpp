// The host side of the calls that run one node column per query node and return k-best lists per row
// (bos_associate_bearings, bos_match_landmarks, bos_match_poses): the rows grouped by node, and a chunk's
// downloaded lists scattered to the caller's order. Pure host code (tests/row_lists_check.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace bos {

// The rows of a call grouped by their node: the nodes in the order of their first row, a node's rows in the
// call's order
struct RowGroups {
    std::vector<int32_t> nodes;
    std::vector<std::vector<int32_t>> members;
};

// node: [n] ids in [0, n_nodes)
inline RowGroups group_rows_by_node(int32_t n, const int32_t* node, size_t n_nodes) {
    RowGroups G;
    std::vector<int32_t> group_of(n_nodes, -1);
    for (int32_t q = 0; q < n; ++q) {
        int32_t& g = group_of[node[q]];
        if (g < 0) {
            g = (int32_t)G.nodes.size();
            G.nodes.push_back(node[q]);
            G.members.emplace_back();
        }
        G.members[g].push_back(q);
    }
    return G;
}

// (the chunk's row, the query that receives it)
typedef std::pair<int32_t, int32_t> RowDest;

// A chunk's download [rows][kmax][stride] to out [n][k][width] in the caller's order: the first k entries of a
// row's list, the first `width` values of an entry, to every query of dst that receives the row (k <= kmax,
// width <= stride). Nothing else of out is written.
template <class T>
void scatter_lists(const T* chunk, size_t kmax, size_t stride, const std::vector<RowDest>& dst, size_t k, size_t width, T* out) {
    for (const RowDest& rq : dst)
        for (size_t j = 0; j < k; ++j)
            std::copy_n(chunk + ((size_t)rq.first * kmax + j) * stride, width, out + ((size_t)rq.second * k + j) * width);
}

}  // namespace bos
