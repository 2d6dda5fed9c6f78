// Headless drop-in for executables/bearing_only_slam.cpp (reference :40-116).
// Usage: bearing_only_slam <dataset_fname> [--iters N] [--lm] [--fp32] [--dense|--schur] [--dump out.g2o]
//                          [--ppm out.ppm] [--check-edges K] [--anchor map.g2o --anchor-sigma S] [--quiet]
// --anchor FILE.g2o: the known-map run. Every landmark whose id also occurs in FILE gets a prior
// (bos_set_priors) at FILE's position with information I / S^2 (--anchor-sigma S, default 0.1); the count and,
// after the run, the priors' sum of rho are printed.
// --lm: Levenberg-Marquardt (bos_optimize, at most --iters iterations, it stops by itself) instead of
// the fixed count of Gauss-Newton steps; one line per iteration.
// --check-edges K: after the run, the K (1 .. 8) bearings and odometry edges with the largest normalised residual
// (bos_edge_consistency): edge index, node ids, e, w2 and the redundancy number, one line per edge.
// Same flow as the reference's main: parse_g2o, default the fixed pose, triangulate the
// landmarks, construct the Solver, then iterate (the reference's Tab press = 50 iterations,
// :93-99). The OpenCV window is replaced by a per-iteration chi^2 line, an optional g2o dump and
// an optional PPM rendering of the initial and final states (utils/draw_utils.cpp without OpenCV).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../host/draw_ppm.hpp"
#include "../host/g2o_utils.hpp"
#include "../host/prior.hpp"
#include "../host/solver.hpp"
#include "../host/triangulation.hpp"

using namespace proj02;

int main(int argc, char** argv) {
    if (argc < 2) {
        std::cout << "usage: bearing_only_slam <dataset_fname> [--iters N] [--lm] [--fp32] [--dense|--schur] [--dump out.g2o] "
                     "[--ppm out.ppm] [--check-edges K] [--anchor map.g2o --anchor-sigma S] [--quiet]"
                  << std::endl;
        return 1;
    }
    int iters = 50, check_edges = 0;
    bool quiet = false, lm = false;
    std::string dump, ppm, anchor;
    double anchor_sigma = 0.1;
    bos_options opt;
    bos_default_options(&opt);
    for (int i = 2; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--iters") && i + 1 < argc) iters = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--lm")) lm = true;
        else if (!std::strcmp(argv[i], "--fp32")) opt.precision = BOS_FP32;
        else if (!std::strcmp(argv[i], "--dense")) opt.solver = BOS_SOLVER_DENSE_CHOL;
        else if (!std::strcmp(argv[i], "--schur")) opt.solver = BOS_SOLVER_SCHUR;
        else if (!std::strcmp(argv[i], "--dump") && i + 1 < argc) dump = argv[++i];
        else if (!std::strcmp(argv[i], "--ppm") && i + 1 < argc) ppm = argv[++i];
        else if (!std::strcmp(argv[i], "--check-edges") && i + 1 < argc) check_edges = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--anchor") && i + 1 < argc) anchor = argv[++i];
        else if (!std::strcmp(argv[i], "--anchor-sigma") && i + 1 < argc) anchor_sigma = std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--quiet")) quiet = true;
        else { std::cerr << "unknown argument " << argv[i] << std::endl; return 1; }
    }
    State state(300, 200);
    BearingObservationVector bearings;
    OdometryObservationVector odometries;
    int fixed_pose_id = -1;
    float bound = 0;
    if (parse_g2o(argv[1], state, bearings, odometries, fixed_pose_id, bound)) {
        std::cerr << "cannot read " << argv[1] << std::endl;
        return 1;
    }
    if (fixed_pose_id < 0) fixed_pose_id = state.default_pose_id();
    triangulate_landmarks(state, bearings, !quiet);
    auto render = [&](const State& st, const std::string& path) {
        PpmImage img(800, 800);
        draw_state_ppm(img, st, odometries, bound);
        if (write_ppm(path, img)) std::cerr << "cannot write " << path << std::endl;
    };
    if (!ppm.empty()) render(state, ppm.substr(0, ppm.rfind('.')) + "_initial.ppm");
    try {
        Solver solver(state, bearings, odometries, fixed_pose_id, &opt);
        // the anchored landmarks (stix), their means and the information, as bos_set_priors takes them
        std::vector<int32_t> anchored;
        std::vector<double> anchor_mean, anchor_omega;
        if (!anchor.empty()) {
            if (!(anchor_sigma > 0.0)) throw std::runtime_error("--anchor-sigma must be positive");
            State map(300, 200);
            BearingObservationVector mb;
            OdometryObservationVector mo;
            int mfixed = -1;
            float mbound = 0;
            if (parse_g2o(anchor, map, mb, mo, mfixed, mbound)) throw std::runtime_error("cannot read " + anchor);
            const double w = 1.0 / (anchor_sigma * anchor_sigma);
            const AssociationVec& ids = state.landmark_ids();
            for (int l = 0; l < (int)ids.size(); ++l) {
                LMPos m;
                try {
                    m = map.get_landmark_by_id(ids[l]);
                } catch (const std::out_of_range&) {
                    continue;
                }
                anchored.push_back(l);
                anchor_mean.insert(anchor_mean.end(), {m.x, m.y});
                anchor_omega.insert(anchor_omega.end(), {w, 0.0, 0.0, w});
            }
            if (bos_set_priors(solver.handle(), 0, nullptr, nullptr, nullptr, (int32_t)anchored.size(), anchored.data(),
                               anchor_mean.data(), anchor_omega.data()) != BOS_OK)
                throw std::runtime_error(bos_last_error());
            std::printf("anchored %d of %d landmarks to %s (sigma %g)\n", (int)anchored.size(), (int)ids.size(), anchor.c_str(),
                        anchor_sigma);
        }
        if (lm) {
            bos_lm_options lo;
            bos_lm_default_options(&lo);
            lo.max_iterations = iters;
            std::vector<bos_lm_iteration> trace(iters > 0 ? iters : 0);
            bos_lm_result res;
            if (bos_optimize(solver.handle(), &lo, &res, trace.data(), (int32_t)trace.size()) != BOS_OK)
                throw std::runtime_error(bos_last_error());
            if (!quiet) {
                for (int it = 0; it < res.iterations; ++it) {
                    const bos_lm_iteration& r = trace[it];
                    std::printf("iter %3d  cost %.9g  trial %.9g  gain %.3g  lambda %.3g  max|dx| %.3g  %s\n", it, r.cost,
                                r.cost_trial, r.gain, r.lambda, r.max_abs_dx, r.accepted ? "accepted" : "rejected");
                }
                std::printf("stopped after %d iterations (%d accepted, %d rejected), reason %d, cost %.9g -> %.9g\n",
                            res.iterations, res.accepted, res.rejected, res.reason, res.cost_initial, res.cost_final);
            }
        }
        for (int it = 0; it < iters && !lm; ++it) {
            solver.step();
            const bos_step_stats& s = solver.last_stats();
            if (!quiet)
                std::printf("iter %3d  chi2 %.9g  robust %d  max|dx| %.3g  J+H %.3f ms  solve %.3f ms\n", it, s.chi2,
                            s.n_robust, s.max_abs_dx, s.t_linearize_ms, s.t_solve_ms);
        }
        if (!anchor.empty()) {   // sum of rho = e^T Omega e over the priors at the final state
            const State& final_state = solver.state;   // the reading overload: a write would re-upload the state
            const LMPosVector& lms = final_state.landmarks_vec();
            const double w = 1.0 / (anchor_sigma * anchor_sigma);
            double rho = 0.0;
            for (size_t i = 0; i < anchored.size(); ++i) {
                const double u[3] = {w, 0.0, w};
                rho += bos::prior_landmark_rho<double>(lms[anchored[i]].x, lms[anchored[i]].y, &anchor_mean[2 * i], u);
            }
            std::printf("anchors: sum of rho %.9g over %d priors\n", rho, (int)anchored.size());
        }
        if (check_edges != 0) {
            const int k = check_edges;
            std::vector<int32_t> cb(8, -1), co(8, -1);
            std::vector<double> cbw(8), cbe(8), cow(8), coe(24), rb(bearings.size()), ro(odometries.size());
            int32_t nb = 0, no = 0;
            if (bos_edge_consistency(solver.handle(), 0.0, 0.0, k, cb.data(), cbw.data(), cbe.data(), nullptr, &nb, co.data(), cow.data(),
                                     coe.data(), nullptr, &no, nullptr, nullptr, rb.data(), nullptr, nullptr, ro.data(), nullptr) != BOS_OK)
                throw std::runtime_error(bos_last_error());
            std::printf("worst bearings (of %d with a finite w2):\n", nb);
            for (int j = 0; j < k && cb[j] >= 0; ++j)
                std::printf("  bearing %d  pose %d  landmark %d  e %.6g  w2 %.6g  redundancy %.6g\n", cb[j], bearings[cb[j]].get_pose_id(),
                            bearings[cb[j]].get_lm_id(), cbe[j], cbw[j], rb[cb[j]]);
            std::printf("worst odometry edges (of %d with a finite w2):\n", no);
            for (int j = 0; j < k && co[j] >= 0; ++j)
                std::printf("  odometry %d  pose %d  pose %d  e (%.6g, %.6g, %.6g)  w2 %.6g  redundancy %.6g\n", co[j],
                            odometries[co[j]].get_source_id(), odometries[co[j]].get_dest_id(), coe[3 * j], coe[3 * j + 1], coe[3 * j + 2],
                            cow[j], ro[co[j]]);
        }
        if (!ppm.empty()) render(solver.state, ppm);
        if (!dump.empty() && write_g2o(dump, solver.state, bearings, odometries, fixed_pose_id, true)) {
            std::cerr << "cannot write " << dump << std::endl;
            return 1;
        }
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 2;
    }
    return 0;
}
