// Stand-alone check of csrc/host/row_lists.hpp on the host (built with AddressSanitizer and UBSan by
// tests/test_row_lists_sanitized.py): the grouping against a brute-force regrouping on random node lists
// (duplicates, a single node, every row its own node, no row), and the scatter against a direct triple loop
// for every k, stride and width the calls use, with every cell that is not addressed left as it was.
#include <cstdio>
#include <random>
#include <vector>

#include "../prb-project-bearing-only-slam_amd/csrc/host/row_lists.hpp"

namespace {

int failures = 0, cases = 0;

void expect(bool ok, const char* what) {
    ++cases;
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

// the nodes in the order of their first row, and per node its rows in the call's order, by searching
void check_groups(const std::vector<int32_t>& node, size_t n_nodes, const char* what) {
    const bos::RowGroups G = bos::group_rows_by_node((int32_t)node.size(), node.data(), n_nodes);
    std::vector<int32_t> first;
    for (int32_t v : node) {
        bool seen = false;
        for (int32_t f : first) seen |= f == v;
        if (!seen) first.push_back(v);
    }
    bool ok = G.nodes == first && G.members.size() == first.size();
    for (size_t g = 0; g < first.size() && ok; ++g) {
        std::vector<int32_t> rows;
        for (size_t q = 0; q < node.size(); ++q)
            if (node[q] == first[g]) rows.push_back((int32_t)q);
        ok = G.members[g] == rows;
    }
    expect(ok, what);
}

void grouping(std::mt19937_64& rng) {
    check_groups({}, 5, "no row");
    check_groups({3}, 4, "one row");
    check_groups({2, 2, 2, 2, 2}, 3, "a single node");
    check_groups({4, 3, 2, 1, 0}, 5, "every row its own node");
    check_groups({1, 0, 1, 0, 1, 1, 0}, 2, "two nodes interleaved");
    for (int t = 0; t < 60; ++t) {
        const size_t n_nodes = 1 + rng() % 12;
        std::vector<int32_t> node(rng() % 40);
        for (int32_t& v : node) v = (int32_t)(rng() % n_nodes);
        check_groups(node, n_nodes, "random node list");
    }
}

// out [n][k][width] from chunk [rows][kmax][stride] by the direct triple loop; the rest of out keeps its fill
template <class T>
void check_scatter(std::mt19937_64& rng, size_t k, size_t stride, size_t width, bool one_row) {
    const size_t kmax = 8, rows = one_row ? 1 : 1 + rng() % 5, n = rows + 1 + rng() % 6;
    std::vector<T> chunk(rows * kmax * stride);
    for (size_t i = 0; i < chunk.size(); ++i) chunk[i] = (T)(i + 1);
    // one_row: a landmark column's one row to a subset of the queries; else each row to a query of its own
    std::vector<int32_t> query(n);
    for (size_t q = 0; q < n; ++q) query[q] = (int32_t)q;
    std::shuffle(query.begin(), query.end(), rng);
    std::vector<bos::RowDest> dst;
    const size_t receivers = one_row ? 1 + rng() % n : rows;
    for (size_t i = 0; i < receivers; ++i) dst.emplace_back(one_row ? 0 : (int32_t)i, query[i]);
    const T fill = (T)-7;
    std::vector<T> out(n * k * width, fill), want(n * k * width, fill);
    for (const bos::RowDest& rq : dst)
        for (size_t j = 0; j < k; ++j)
            for (size_t w = 0; w < width; ++w)
                want[((size_t)rq.second * k + j) * width + w] = chunk[((size_t)rq.first * kmax + j) * stride + w];
    // exactly sized buffers: a read or write past either end is the sanitizer's to report
    bos::scatter_lists(chunk.data(), kmax, stride, dst, k, width, out.data());
    expect(out == want, "scatter");
}

void scatter(std::mt19937_64& rng) {
    const size_t ks[3] = {1, 4, 8}, strides[3] = {1, 3, 9}, widths[5] = {1, 2, 3, 4, 9};
    for (size_t k : ks)
        for (size_t stride : strides)
            for (size_t width : widths) {
                if (width > stride) continue;   // an entry holds at most its stride
                for (int one_row = 0; one_row < 2; ++one_row)
                    for (int t = 0; t < 3; ++t) {
                        check_scatter<double>(rng, k, stride, width, one_row != 0);
                        check_scatter<int32_t>(rng, k, stride, width, one_row != 0);
                    }
            }
    std::vector<double> chunk(8, 1.0), out(4, -7.0);
    bos::scatter_lists(chunk.data(), 8, 1, {}, 4, 1, out.data());
    expect(out == std::vector<double>(4, -7.0), "no destination");
}

}  // namespace

int main() {
    std::mt19937_64 rng(20240917);
    grouping(rng);
    scatter(rng);
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
