// Stand-alone check of csrc/host/associate.hpp on the host (built with AddressSanitizer and UBSan by
// tests/test_associate_sanitized.py): the register list of the device's selection (assoc_top_insert, merged
// the way the kernels merge) against a plain sort over (nis, stix), with ties, values outside the gate,
// infinities and NaNs; nis against e * e / S; the argument rules.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../prb-project-bearing-only-slam_amd/csrc/host/associate.hpp"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

// the kernels' selection on the host: `lists` register lists, landmark l to list l % lists, merged pairwise
std::vector<int32_t> select_like_device(const std::vector<double>& nis, double gate, int lists, int* count) {
    std::vector<bos::AssocTop> top(lists);
    for (bos::AssocTop& t : top) bos::assoc_top_clear(t);
    *count = 0;
    for (size_t l = 0; l < nis.size(); ++l)
        if (bos::assoc_inside(nis[l], gate)) {
            bos::assoc_top_insert(top[l % lists], nis[l], (int32_t)l);
            ++*count;
        }
    for (int stride = lists / 2; stride > 0; stride >>= 1)
        for (int t = 0; t < stride; ++t)
            for (int i = 0; i < bos::kAssocMaxK; ++i) bos::assoc_top_insert(top[t], top[t + stride].nis[i], top[t + stride].l[i]);
    return std::vector<int32_t>(top[0].l, top[0].l + bos::kAssocMaxK);
}

std::vector<int32_t> select_by_sort(const std::vector<double>& nis, double gate, int* count) {
    std::vector<int32_t> in;
    for (size_t l = 0; l < nis.size(); ++l)
        if (bos::assoc_inside(nis[l], gate)) in.push_back((int32_t)l);
    *count = (int)in.size();
    std::sort(in.begin(), in.end(), [&](int32_t x, int32_t y) { return bos::assoc_less(nis[x], x, nis[y], y); });
    in.resize(bos::kAssocMaxK, bos::kAssocNone);
    return in;
}

}  // namespace

int main() {
    std::mt19937_64 rng(11);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    int cases = 0;
    for (int n : {0, 1, 5, 8, 9, 63, 64, 257, 1024, 2109})
        for (int lists : {1, 4, 64, 256})
            for (double gate : {inf, 6.63, 0.5, 1e-9}) {
                std::vector<double> nis(n);
                for (double& v : nis) {
                    const unsigned kind = rng() % 16;
                    // a few levels only, so equal values are common; some infinities and NaNs
                    v = kind == 0 ? inf : kind == 1 ? nan : kind == 2 ? 0.0 : 0.25 * (double)(rng() % 40);
                }
                int c_dev = -1, c_ref = -2;
                expect(select_like_device(nis, gate, lists, &c_dev) == select_by_sort(nis, gate, &c_ref) && c_dev == c_ref,
                       "the merged register lists equal the sorted selection");
                ++cases;
            }
    std::uniform_real_distribution<double> u(-3.2, 3.2);
    for (int i = 0; i < 1000; ++i) {
        const double e = u(rng), var = 0.001 + std::abs(u(rng)), omega = 0.5 + std::abs(u(rng));
        const double S = bos::assoc_innovation_var(var, omega);
        volatile double ee = e * e;   // the product rounded on its own
        expect(S == var + 1.0 / omega && bos::assoc_nis(e, S) == ee / S, "nis is (e * e) / S in IEEE arithmetic");
    }
    expect(!bos::assoc_inside(nan, inf) && !bos::assoc_inside(inf, inf) && bos::assoc_inside(0.0, inf) && !bos::assoc_inside(2.0, 1.0),
           "the gate drops what is not finite");
    const int32_t pose[2] = {0, 2}, bad_pose[2] = {0, 3};
    const double z[2] = {0.1, -7.0}, bad_z[2] = {0.1, inf}, om[2] = {1.0, 25.0}, bad_om[2] = {1.0, 0.0};
    expect(!bos::assoc_bad_argument(3, 2, pose, z, om, inf, 8) && !bos::assoc_bad_argument(3, 2, pose, z, nullptr, 1.0, 1) &&
               !bos::assoc_bad_argument(3, 0, nullptr, nullptr, nullptr, 1.0, 1),
           "valid arguments pass");
    expect(bos::assoc_bad_argument(3, 2, bad_pose, z, om, 1.0, 4) && bos::assoc_bad_argument(3, 2, pose, bad_z, om, 1.0, 4) &&
               bos::assoc_bad_argument(3, 2, pose, z, bad_om, 1.0, 4) && bos::assoc_bad_argument(3, 2, pose, z, om, nan, 4) &&
               bos::assoc_bad_argument(3, 2, pose, z, om, 0.0, 4) && bos::assoc_bad_argument(3, 2, pose, z, om, 1.0, 0) &&
               bos::assoc_bad_argument(3, 2, pose, z, om, 1.0, 9) && bos::assoc_bad_argument(3, -1, pose, z, om, 1.0, 4) &&
               bos::assoc_bad_argument(3, 2, nullptr, z, om, 1.0, 4),
           "invalid arguments are refused");
    std::printf("associate_check: %d selections, %d failures\n", cases, failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
