// CPU driver of tests/test_ibm_bodies.py: the body tables and the step plan of xlb_amd/csrc/ibm_bodies.hpp for the commands read
// from stdin.
//   tables N NB  FIRST COUNT MOVING CX CY CZ  (NB times)  -> "error TEXT", or the six lines
//        flags ANY_MOVING ANY_PRESCRIBED ANY_DYNAMIC
//        chunk0 ...            kind ...
//        chunks BODY:FIRST:COUNT ...
//        move_id VALUExRUN ... (run-length: -1x3 0x5 = three markers of no moving body, then five of body 0)
//        rest ...              (18 doubles per body)
//   nulls NB                   -> ibm_check_bodies with null arrays: "error TEXT" or "ok"
//   plan ANY_MOVING ANY_PRESCRIBED ANY_DYNAMIC DYNAMICS_SET VIRTUAL_ON CONTACT_ON RECORDING_POSES
//                              -> "POSE LIVE STAGED INTEGRATOR MOVE": live / rest / staged, 0 / 1, 0 / 1,
//                                 none / integrate / contact+radius / contact+null, 0 / 1
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "ibm_bodies.hpp"

using namespace xlb;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "tables") {
      long long n = 0;
      int nb = 0;
      in >> n >> nb;
      std::vector<int64_t> first, count;
      std::vector<int> moving;
      std::vector<double> centre0;
      for (int i = 0; i < nb; ++i) {
        long long f = 0, c = 0;
        int m = 0;
        double x = 0, y = 0, z = 0;
        in >> f >> c >> m >> x >> y >> z;
        first.push_back(f);
        count.push_back(c);
        moving.push_back(m);
        centre0.insert(centre0.end(), {x, y, z});
      }
      first.resize(first.size() + 1);  // (data() of an empty vector may be null, which is "null argument")
      count.resize(count.size() + 1);
      moving.resize(moving.size() + 1);
      centre0.resize(centre0.size() + 1);
      const IbmBodyTables t = ibm_body_tables(n, nb, first.data(), count.data(), moving.data(), centre0.data());
      if (!t.error.empty()) {
        std::printf("error %s\n", t.error.c_str());
        continue;
      }
      std::printf("flags %d %d %d\nchunk0", t.any_moving, t.any_prescribed, t.any_dynamic);
      for (int32_t c : t.chunk0) std::printf(" %d", c);
      std::printf("\nkind");
      for (int32_t k : t.kind) std::printf(" %d", k);
      std::printf("\nchunks");
      for (const IbmLoadChunk& c : t.chunks) std::printf(" %d:%d:%d", c.body, c.first, c.count);
      std::printf("\nmove_id");
      for (size_t k = 0; k < t.move_id.size();) {
        size_t e = k;
        while (e < t.move_id.size() && t.move_id[e] == t.move_id[k]) ++e;
        std::printf(" %dx%zu", t.move_id[k], e - k);
        k = e;
      }
      std::printf("\nrest");
      for (double v : t.rest) std::printf(" %.17g", v);
      std::printf("\n");
    } else if (what == "nulls") {
      int nb = 0;
      in >> nb;
      const std::string e = ibm_check_bodies(1000, nb, nullptr, nullptr, nullptr, nullptr);
      std::printf("%s\n", e.empty() ? "ok" : ("error " + e).c_str());
    } else if (what == "plan") {
      IbmStepPlan p;
      in >> p.any_moving >> p.any_prescribed >> p.any_dynamic >> p.dynamics_set >> p.virtual_on >> p.contact_on >> p.recording_poses;
      const IbmPoseSource s = p.pose_source();
      const IbmIntegrator g = p.integrator();
      std::printf("%s %d %d %s %d\n", s == IbmPoseSource::LIVE ? "live" : s == IbmPoseSource::REST ? "rest" : "staged", p.use_live(), p.needs_staged(),
                  g == IbmIntegrator::NONE ? "none" : g == IbmIntegrator::PLAIN ? "integrate" : p.passes_radius() ? "contact+radius" : "contact+null", p.moves());
    }
  }
  return 0;
}
