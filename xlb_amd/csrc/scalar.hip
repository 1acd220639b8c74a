// libxlbhip: scalar transport.  The object owns the boundary tables of the coupled step (the fluid's: a BcTables like a stepper's,
// stepper_tables.hpp; and the scalar's rule and value by bc id); a step enqueues the coupled kernel and the fluid's outflow pass on the
// context's compute stream, and nothing here waits for the device.
#include <cmath>
#include <vector>

#include "scalar_launch.hpp"
#include "stepper_tables.hpp"

using namespace xlb;

struct xlbhip_scalar : RowStepper {  // (bc: the fluid's)
  int collision = 0;
  DeviceBuf sc_rule;   // uint8 [256] SCALAR_*
  DeviceBuf sc_value;  // [256] compute dtype
  bool forced = false;
  ScalarCoupling cp{{0, 0, 0}, {0, 0, 0}, 0.0};
  double smag_cs = 0.17;
};

namespace xlb {

static int scalar_q(int lattice) { return 2 * lattice_d(lattice) + 1; }

static int upload_rules(xlbhip_scalar* s, const std::vector<uint8_t>& rule, const std::vector<double>& value) {
  if (int rc = upload_bytes(rule.data(), 256, s->sc_rule)) return rc;
  return upload_values(s->cdt, value, s->sc_value);
}

static int check_scalar_fields(const xlbhip_scalar* s, const xlbhip_field* fa, const xlbhip_field* fb, const xlbhip_field* ga, const xlbhip_field* gb,
                               const xlbhip_field* bcm, const xlbhip_field* miss) {
  XLB_REQUIRE(s && fa && fb && ga && gb, "null argument");
  XLB_REQUIRE(fa != fb && ga != gb, "f_0 / f_1 and g_0 / g_1 must be different fields (double buffering)");
  if (int rc = check_row_fields("scalar transport", "population fields", lattice_q(s->lattice), s->sdt, {fa, fb}, true)) return rc;
  if (int rc = check_row_fields("scalar transport", "scalar population fields", scalar_q(s->lattice), s->sdt, {ga, gb}, true)) return rc;
  XLB_REQUIRE(same_grid(ga, fa), "scalar transport: the fields of a step must share one grid");
  return check_single_rank_grid("scalar transport", "step kernel", s->lattice, s->bc.n_bc, fa, bcm, miss);
}

static int check_omegas(double omega, double omega_s) {
  if (int rc = check_relaxation("omega", omega)) return rc;
  return check_relaxation("omega_scalar", omega_s);
}

// one coupled step (f, g)(t) -> (f, g)(t + 1), then the auxiliary data of the fluid's ExtrapolationOutflowBC cells
static int scalar_step_once(xlbhip_scalar* s, const xlbhip_field* fs, xlbhip_field* fd, const xlbhip_field* gs, xlbhip_field* gd, const xlbhip_field* bcm,
                            const xlbhip_field* miss, double omega, double omega_s) {
  xlbhip_ctx* c = s->ctx;
  touch(fd);
  touch(gd);
  ScalarLaunch q;
  StepLaunch& p = q.f;
  p = bc_launch(c, s->bc, s->cdt, s->sdt, bcm, miss, fs);
  p.src = fs->data;
  p.dst = fd->data;
  p.plane_stride = fs->plane_stride;
  p.omega = omega;
  p.smag_cs = s->smag_cs;
  p.vec = (int)opt(c, "vec", 0);
  p.has_bc = s->bc.n_bc > 0 ? 2 : 0;
  q.gsrc = gs->data;
  q.gdst = gd->data;
  q.g_plane_stride = gs->plane_stride;
  q.sc_rule = s->sc_rule.get<uint8_t>();
  q.sc_value = s->sc_value.get();
  q.cp = s->cp;
  q.omega_s = omega_s;
  const int coll = s->collision | (s->forced ? COLL_FORCED : 0);
  if (int rc = launch_for_lattice(s->lattice, launch_scalar_d2q9, launch_scalar_d3q19, launch_scalar_d3q27, q, coll)) return rc;
  return outflow_aux(c, s->lattice, s->cdt, s->bc, CellTables(), fs, fd, bcm, miss);
}

}  // namespace xlb

extern "C" {

int xlbhip_scalar_create(xlbhip_ctx* c, int lattice, int collision, int cdt, int sdt, int n_bc, const xlbhip_bc_desc* bcs, xlbhip_scalar** out) {
  XLB_REQUIRE(collision == XLBHIP_BGK || collision == XLBHIP_KBC || collision == XLBHIP_SMAGORINSKY_LES_BGK, "unknown collision %d", collision);
  XLB_REQUIRE(!(collision == XLBHIP_KBC && lattice == XLBHIP_D3Q19), "Velocity set not supported: D3Q19 has no KBC (reference kbc.py:65-66)");
  const auto refusal = [](int kind) {
    return bc_scalar_accepts(kind) ? nullptr : "scalar transport: bc kind %d (HybridBC, profile walls) is not supported by the coupled step";
  };
  const auto own = [&](xlbhip_scalar& s) {
    s.collision = collision;
    return upload_rules(&s, std::vector<uint8_t>(256, SCALAR_ADIABATIC), std::vector<double>(256, 0.0));
  };
  return create_row_stepper(c, lattice, cdt, sdt, n_bc, bcs, SCALAR_POLICY_SUBJECT, refusal, own, out);
}

int xlbhip_scalar_destroy(xlbhip_scalar* s) { return destroy_drained(s); }

int xlbhip_scalar_set_rules(xlbhip_scalar* s, int n, const int32_t* bc_ids, const int32_t* rules, const double* values) {
  XLB_REQUIRE(s && n >= 0 && (n == 0 || (bc_ids && rules && values)), "bad argument");
  std::vector<uint8_t> rule(256, SCALAR_ADIABATIC);
  std::vector<double> value(256, 0.0);
  for (int i = 0; i < n; ++i) {
    const int id = bc_ids[i];
    XLB_REQUIRE(id >= 1 && id <= 255 && s->bc.kind_host[id] != 0, "scalar rule for bc id %d, which is none of this stepper's boundary conditions", id);
    XLB_REQUIRE(rules[i] >= SCALAR_ADIABATIC && rules[i] <= SCALAR_DO_NOTHING, "unknown scalar rule %d", rules[i]);
    XLB_REQUIRE(!(rules[i] == SCALAR_DIRICHLET && s->bc.kind_host[id] == XLBHIP_BC_FULLWAY_BB),
                "a Dirichlet scalar rule cannot sit on a fullway bounce-back wall (bc id %d): the scalar is bounced fullway there", id);
    XLB_REQUIRE(std::isfinite(values[i]), "scalar rule of bc id %d: value is not finite", id);
    rule[id] = (uint8_t)rules[i];
    value[id] = values[i];
  }
  XLB_HIP(hipSetDevice(s->ctx->device));
  XLB_HIP(hipStreamSynchronize(s->ctx->stream));  // (launches may still read the old tables)
  return upload_rules(s, rule, value);
}

int xlbhip_scalar_set_coupling(xlbhip_scalar* s, const double* force, const double* buoyancy, double reference, double smagorinsky_coef) {
  XLB_REQUIRE(s, "null argument");
  s->forced = force != nullptr || buoyancy != nullptr;
  for (int a = 0; a < 3; ++a) {
    s->cp.force[a] = force ? force[a] : 0.0;
    s->cp.buoyancy[a] = buoyancy ? buoyancy[a] : 0.0;
  }
  s->cp.reference = reference;
  s->smag_cs = smagorinsky_coef;
  return 0;
}

int xlbhip_scalar_init(xlbhip_scalar* s, const xlbhip_field* f_0, const xlbhip_field* phi, double phi0, xlbhip_field* g_0) {
  XLB_REQUIRE(s && f_0 && g_0, "null argument");
  XLB_CHECK_POP(f_0, s->lattice, "scalar_init(f_0)");
  XLB_REQUIRE(is_float(g_0->dtype) && g_0->card == scalar_q(s->lattice) && same_grid(g_0, f_0) && g_0->halo == 0 && f_0->halo == 0,
              "scalar_init: g_0 must be a %d-population float field on f_0's grid, without ghost planes", scalar_q(s->lattice));
  XLB_REQUIRE(!phi || (is_float(phi->dtype) && phi->card == 1 && same_grid(phi, f_0) && phi->halo == 0), "scalar_init: bad scalar field");
  xlbhip_ctx* c = s->ctx;
  XLB_HIP(hipSetDevice(c->device));
  touch(g_0);
  const size_t n = f_0->cells();
  return by_lattice(s->lattice, [&](auto L) {
    return by_compute(s->cdt, [&](auto T) {
      using TT = decltype(T);
      hipLaunchKernelGGL((k_scalar_init<decltype(L), TT>), blocks_for(n), 256, 0, c->stream, view(f_0), view(phi), (TT)phi0, view(g_0), dims(f_0));
      XLB_HIP(hipGetLastError());
      return 0;
    });
  });
}

int xlbhip_scalar_moment(xlbhip_ctx* c, int lattice, int compute_dtype, const xlbhip_field* g, xlbhip_field* phi) {
  XLB_REQUIRE(c && g && phi, "null argument");
  XLB_REQUIRE(lattice_q(lattice) > 0, "unknown lattice %d", lattice);
  XLB_REQUIRE(compute_dtype == XLBHIP_F32 || compute_dtype == XLBHIP_F64, "bad compute dtype %d", compute_dtype);
  XLB_REQUIRE(is_float(g->dtype) && g->card == scalar_q(lattice), "scalar_moment: expected a %d-population float field", scalar_q(lattice));
  XLB_REQUIRE(is_float(phi->dtype) && phi->card == 1 && same_grid(phi, g) && phi->halo == g->halo, "scalar_moment: bad output field");
  XLB_HIP(hipSetDevice(c->device));
  touch(phi);
  const size_t n = g->cells();
  return by_lattice(lattice, [&](auto L) {
    return by_compute(compute_dtype, [&](auto T) {
      using TT = decltype(T);
      hipLaunchKernelGGL((k_scalar_moment<decltype(L), TT>), blocks_for(n), 256, 0, c->stream, view(g), view(phi), dims(g));
      XLB_HIP(hipGetLastError());
      return 0;
    });
  });
}

int xlbhip_scalar_step(xlbhip_scalar* s, const xlbhip_field* f_src, xlbhip_field* f_dst, const xlbhip_field* g_src, xlbhip_field* g_dst,
                       const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega, double omega_scalar, int64_t timestep) {
  (void)timestep;  // (no time-dependent walls in the coupled step)
  if (int rc = check_scalar_fields(s, f_src, f_dst, g_src, g_dst, bc_mask, missing_mask)) return rc;
  if (int rc = check_omegas(omega, omega_scalar)) return rc;
  XLB_HIP(hipSetDevice(s->ctx->device));
  return scalar_step_once(s, f_src, f_dst, g_src, g_dst, bc_mask, missing_mask, omega, omega_scalar);
}

int xlbhip_scalar_run(xlbhip_scalar* s, xlbhip_field* f_a, xlbhip_field* f_b, xlbhip_field* g_a, xlbhip_field* g_b, const xlbhip_field* bc_mask,
                      const xlbhip_field* missing_mask, double omega, double omega_scalar, int64_t first_timestep, int64_t n_steps, int* result_in_b) {
  (void)first_timestep;
  XLB_REQUIRE(result_in_b && n_steps >= 0, "bad argument");
  if (int rc = check_scalar_fields(s, f_a, f_b, g_a, g_b, bc_mask, missing_mask)) return rc;
  if (int rc = check_omegas(omega, omega_scalar)) return rc;
  XLB_HIP(hipSetDevice(s->ctx->device));
  return run_alternating(n_steps, result_in_b, [&](int64_t, bool odd) {
    return odd ? scalar_step_once(s, f_b, f_a, g_b, g_a, bc_mask, missing_mask, omega, omega_scalar)
               : scalar_step_once(s, f_a, f_b, g_a, g_b, bc_mask, missing_mask, omega, omega_scalar);
  });
}

}  // extern "C"
