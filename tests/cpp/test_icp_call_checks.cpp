// test_icp_call_checks.cpp — the order of the refusals of a whole ICP call (host_icp_check.hpp's check_call), on the
// host alone. For each of the five entry points (clipper_hip_icp, clipper_hip_icp_generalized, their robust forms,
// clipper_hip_cloud_icp) a call that is wrong in every rung at once is repaired one rung at a time, in the order the
// entry point tries its refusals; before every repair the message must be that rung's, after the last one empty.
// Prints "icp call checks ok", or a line with FAILED per mismatch. Four-point clouds; g++ -std=c++17 -ffp-contract=off.
#include <cmath>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "host_icp_check.hpp"

using namespace clipper_icp;

namespace {

int failures = 0;

// a call as check_call takes it, every part replaceable
struct Call {
  Family family;
  RobustUse use;
  bool has_params = true, has_robust = true, has_T_out = false, host = true;
  Params p{};
  Robust r{};
  const double* T_init = nullptr;
  HostClouds c{};
};

std::string run(const Call& k) {
  return check_call(k.family, k.use, k.has_params ? &k.p : nullptr, k.has_robust ? &k.r : nullptr, k.has_T_out, k.T_init,
                    k.host ? &k.c : nullptr);
}

struct Rung {
  std::string want;                   // the refusal while this rung is wrong
  std::function<void(Call&)> repair;  // puts this rung right (or wrong in its next way)
};

void ladder(const char* name, Call k, const std::vector<Rung>& rungs) {
  for (size_t i = 0; i < rungs.size(); ++i) {
    const std::string got = run(k);
    if (got != rungs[i].want) {
      std::printf("FAILED %s rung %zu: want \"%s\", got \"%s\"\n", name, i, rungs[i].want.c_str(), got.c_str());
      ++failures;
    }
    rungs[i].repair(k);
  }
  const std::string got = run(k);
  if (!got.empty()) {
    std::printf("FAILED %s: the repaired call is refused: \"%s\"\n", name, got.c_str());
    ++failures;
  }
}

// the data of the calls: good and bad clouds of four points, transforms, normals, covariances
const double GOOD[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
const double BAD[12] = {0, 0, 0, 1, 0, 0, 0, INFINITY, 0, 0, 0, 1};  // coordinate 1 of point 2
const double T_GOOD[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0.5, 0, 0, 1};
const double T_BAD[16] = {1, 0, 0, 0.5, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // entry (3, 0)
const double NORMALS[12] = {0, 0, 1, 0, 0, 1, 0, 1, 0, 1, 0, 0};
const double COV[24] = {1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0, 1};
const double COV_BAD[24] = {1, 0, 0, 1, 0, 1, 1, 0, 0, -1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0, 1};  // point 1: minor 2 = -1

const char* const MAXD = "max_distance must be positive and finite (max_distance = 0)";
const char* const T_ROW = "T_init: the bottom row must be 0 0 0 1 (entry (3, 0) = 0.5)";

// wrong in every rung at once: no T_out, max_distance 0, a bad loss, a null source and target, a bad T_init, nothing of
// what the method reads of the clouds
Call all_wrong(Family family, RobustUse use, int method, bool host) {
  Call k;
  k.family = family, k.use = use, k.host = host;
  k.p = Params{method, 30, 0.0, 1e-6, 1e-6};
  k.r = Robust{9, 0, 0.0, 1.0};
  k.T_init = T_BAD;
  k.c = HostClouds{nullptr, 4, nullptr, 4, nullptr, nullptr, nullptr};
  return k;
}

// the rungs every host-buffer call shares behind the parameters and the robust settings
void clouds_and_transform(std::vector<Rung>& v) {
  v.push_back({"null source point array", [](Call& k) { k.c.P_src = BAD; }});
  v.push_back({"source: non-finite value at coordinate 1 of point 2", [](Call& k) { k.c.P_src = GOOD; }});
  v.push_back({"null target point array", [](Call& k) { k.c.P_tgt = BAD; }});
  v.push_back({"target: non-finite value at coordinate 1 of point 2", [](Call& k) { k.c.P_tgt = GOOD; }});
  v.push_back({T_ROW, [](Call& k) { k.T_init = T_GOOD; }});
}

void robust_rungs(std::vector<Rung>& v) {
  v.push_back({"unknown loss 9 (the losses are 0..4)", [](Call& k) { k.has_robust = false; }});
  v.push_back({"null robust", [](Call& k) { k.has_robust = true, k.r = Robust{1, 0, 0.02, 0.8}; }});
}

void point_plane(const char* name, RobustUse use) {
  std::vector<Rung> v;
  v.push_back({"null T_out", [](Call& k) { k.has_T_out = true; }});
  v.push_back({"method 2 (generalized) takes per-point covariances: call clipper_hip_icp_generalized",
               [](Call& k) { k.p.method = 7; }});
  v.push_back({"unknown method 7", [](Call& k) { k.p.method = clipper_hip::ICP_POINT_TO_PLANE; }});
  v.push_back({MAXD, [](Call& k) { k.p.max_distance = 0.1; }});
  if (use == ROBUST_REQUIRED) robust_rungs(v);
  clouds_and_transform(v);
  v.push_back({"point-to-plane needs the target's normals (N_tgt is null)", [](Call& k) { k.c.N_tgt = NORMALS; }});
  ladder(name, all_wrong(FAMILY_POINT_PLANE, use, clipper_hip::ICP_GENERALIZED, true), v);
}

void generalized(const char* name, RobustUse use) {
  std::vector<Rung> v;
  v.push_back({"null T_out", [](Call& k) { k.has_T_out = true; }});
  v.push_back({"method must be CLIPPER_ICP_GENERALIZED (2) (method = 1)", [](Call& k) { k.p.method = clipper_hip::ICP_GENERALIZED; }});
  v.push_back({MAXD, [](Call& k) { k.p.max_distance = 0.1; }});
  if (use == ROBUST_REQUIRED) robust_rungs(v);
  clouds_and_transform(v);
  v.push_back({"null source covariance array", [](Call& k) { k.c.C_src = COV_BAD; }});
  v.push_back({"source covariances: the matrix of point 1 is not positive definite (leading minor 2 = -1)",
               [](Call& k) { k.c.C_src = COV; }});
  v.push_back({"null target covariance array", [](Call& k) { k.c.C_tgt = COV_BAD; }});
  v.push_back({"target covariances: the matrix of point 1 is not positive definite (leading minor 2 = -1)",
               [](Call& k) { k.c.C_tgt = COV; }});
  ladder(name, all_wrong(FAMILY_GENERALIZED, use, clipper_hip::ICP_POINT_TO_PLANE, true), v);
}

// clipper_hip_cloud_icp: the parameter check goes by the method, robust is checked only when given, no cloud is read
void handles() {
  std::vector<Rung> v;
  v.push_back({"null T_out", [](Call& k) { k.has_T_out = true; }});
  v.push_back({"unknown method 7", [](Call& k) { k.has_params = false; }});
  v.push_back({"null params", [](Call& k) { k.has_params = true, k.p.method = clipper_hip::ICP_POINT_TO_PLANE; }});
  v.push_back({MAXD, [](Call& k) { k.p.max_distance = 0.1; }});
  v.push_back({"unknown loss 9 (the losses are 0..4)", [](Call& k) { k.r = Robust{0, 0, 0.0, 0.5}; }});
  v.push_back({T_ROW, [](Call& k) { k.T_init = nullptr; }});
  ladder("cloud_icp", all_wrong(FAMILY_BY_METHOD, ROBUST_OPTIONAL, 7, false), v);

  // a generalized method is accepted, and what refuses its parameters is check_generalized_params
  Call k = all_wrong(FAMILY_BY_METHOD, ROBUST_OPTIONAL, clipper_hip::ICP_GENERALIZED, false);
  k.has_T_out = true, k.has_robust = false, k.T_init = nullptr;
  k.p.max_distance = 0.1, k.p.max_iterations = 1001;
  const std::string want = check_generalized_params(&k.p);
  if (want.empty() || run(k) != want || check_params(&k.p) == want) {
    std::printf("FAILED cloud_icp: generalized parameters: want \"%s\", got \"%s\"\n", want.c_str(), run(k).c_str());
    ++failures;
  }
  k.p.max_iterations = 30;
  // ... and with them right the call passes: the method, and the absent robust (a bad one would be refused)
  if (!run(k).empty()) {
    std::printf("FAILED cloud_icp: a generalized call without robust is refused: \"%s\"\n", run(k).c_str());
    ++failures;
  }
  k.has_robust = true;
  if (run(k) != "unknown loss 9 (the losses are 0..4)") {
    std::printf("FAILED cloud_icp: a bad robust that is given passes: \"%s\"\n", run(k).c_str());
    ++failures;
  }
}

}  // namespace

int main() {
  point_plane("icp", ROBUST_ABSENT);
  point_plane("icp_robust", ROBUST_REQUIRED);
  generalized("icp_generalized", ROBUST_ABSENT);
  generalized("icp_generalized_robust", ROBUST_REQUIRED);
  handles();
  if (failures) return 1;
  std::printf("icp call checks ok\n");
  return 0;
}
