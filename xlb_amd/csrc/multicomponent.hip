// libxlbhip: two-component Shan-Chen flow.  The object owns the boundary tables of the step (a BcTables like a stepper's,
// stepper_tables.hpp), the two wall-density tables by bc id and the two density fields (one value per cell each in the compute dtype,
// allocated at first use); a step enqueues k_mix_density and k_mix_step on the context's compute stream, and nothing here waits for
// the device.
#include <cmath>
#include <vector>

#include "multicomponent_launch.hpp"
#include "stepper_tables.hpp"

using namespace xlb;

struct xlbhip_multicomponent : RowStepper {
  DeviceBuf wall_a, wall_b;  // [256] compute dtype: rho_w by bc id
  DeviceBuf rho_a, rho_b;    // [rho_cells] compute dtype
  size_t rho_cells = 0;
  double g_aa = 0.0, g_ab = 0.0, g_bb = 0.0;
  double force[3] = {0, 0, 0};
};

namespace xlb {

// The two population fields of a state, with their double-buffering partners (or nullptr), and the masks
static int check_mix_grid(const xlbhip_multicomponent* s, const xlbhip_field* fa, const xlbhip_field* fa_other, const xlbhip_field* fb,
                          const xlbhip_field* fb_other, const xlbhip_field* bcm, const xlbhip_field* miss) {
  if (int rc = check_row_fields("multicomponent", "population fields", lattice_q(s->lattice), s->sdt, {fa, fa_other, fb, fb_other}, true)) return rc;
  return check_single_rank_grid("multicomponent", "step kernel", s->lattice, s->bc.n_bc, fa, bcm, miss);
}

// an output of `card` planes in the compute dtype on f's grid, or nullptr
static int check_mix_output(const xlbhip_multicomponent* s, const char* name, const xlbhip_field* out, int card, const xlbhip_field* f) {
  if (!out) return 0;
  XLB_REQUIRE(out->dtype == s->cdt && out->card == card && same_grid(out, f) && out->halo == 0,
              "multicomponent: %s must be a field of cardinality %d in the compute dtype on f's grid, without ghost planes", name, card);
  return 0;
}

static int ensure_densities(xlbhip_multicomponent* s, const xlbhip_field* f) {
  if (s->rho_a && s->rho_b && s->rho_cells == f->cells()) return 0;
  s->rho_cells = 0;
  XLB_HIP(s->rho_a.alloc(f->cells() * dtype_size(s->cdt)));  // (hipFree of the old ones waits for the launches that read them)
  XLB_HIP(s->rho_b.alloc(f->cells() * dtype_size(s->cdt)));
  s->rho_cells = f->cells();
  return 0;
}

static MixLaunch mix_launch(const xlbhip_multicomponent* s, const xlbhip_field* fa, const xlbhip_field* fb, const xlbhip_field* bcm, const xlbhip_field* miss,
                            double omega_a, double omega_b) {
  MixLaunch q = {};
  StepLaunch& p = q.f;
  p = bc_launch(s->ctx, s->bc, s->cdt, s->sdt, bcm, miss, fa);
  p.src = fa->data;
  p.plane_stride = fa->plane_stride;
  p.omega = omega_a;
  p.vec = 1;
  p.has_bc = s->bc.n_bc > 0 ? 1 : 0;
  q.src_b = fb->data;
  q.omega_b = omega_b;
  q.rho_a = s->rho_a.get();
  q.rho_b = s->rho_b.get();
  q.wall_a = s->wall_a.get();
  q.wall_b = s->wall_b.get();
  q.g_aa = s->g_aa;
  q.g_ab = s->g_ab;
  q.g_bb = s->g_bb;
  for (int k = 0; k < 3; ++k) q.force[k] = s->force[k];
  return q;
}

static int mix_dispatch(const xlbhip_multicomponent* s, const MixLaunch& q, MixKernel which) {
  return launch_for_lattice(s->lattice, launch_multicomponent_d2q9, launch_multicomponent_d3q19, launch_multicomponent_d3q27, q, which);
}

// one step (f^A, f^B)(t) -> (t + 1): both densities of the post-streaming state, then the step that reads them
static int mix_step_once(xlbhip_multicomponent* s, const xlbhip_field* fa_src, xlbhip_field* fa_dst, const xlbhip_field* fb_src, xlbhip_field* fb_dst,
                         const xlbhip_field* bcm, const xlbhip_field* miss, double omega_a, double omega_b) {
  touch(fa_dst);
  touch(fb_dst);
  MixLaunch q = mix_launch(s, fa_src, fb_src, bcm, miss, omega_a, omega_b);
  q.f.dst = fa_dst->data;
  q.dst_b = fb_dst->data;
  if (int rc = mix_dispatch(s, q, MixKernel::density)) return rc;
  return mix_dispatch(s, q, MixKernel::step);
}

static int check_mix_step(xlbhip_multicomponent* s, const xlbhip_field* fa_0, const xlbhip_field* fa_1, const xlbhip_field* fb_0, const xlbhip_field* fb_1,
                          const xlbhip_field* bcm, const xlbhip_field* miss, double omega_a, double omega_b) {
  XLB_REQUIRE(s && fa_0 && fa_1 && fb_0 && fb_1, "null argument");
  XLB_REQUIRE(fa_0 != fa_1 && fa_0 != fb_0 && fa_0 != fb_1 && fa_1 != fb_0 && fa_1 != fb_1 && fb_0 != fb_1,
              "the four population fields must be different fields (two components, double buffering)");
  if (int rc = check_mix_grid(s, fa_0, fa_1, fb_0, fb_1, bcm, miss)) return rc;
  if (int rc = check_relaxation("omega_A", omega_a)) return rc;
  if (int rc = check_relaxation("omega_B", omega_b)) return rc;
  XLB_HIP(hipSetDevice(s->ctx->device));
  return ensure_densities(s, fa_0);
}

// k_mix_density into the object's fields, then rho_A, rho_B, u and / or the forces of the post-streaming state (each output may be
// nullptr)
static int mix_outputs(xlbhip_multicomponent* s, const xlbhip_field* fa, const xlbhip_field* fb, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask,
                       xlbhip_field* rho_a, xlbhip_field* rho_b, xlbhip_field* u, xlbhip_field* force_a, xlbhip_field* force_b) {
  XLB_REQUIRE(s && fa && fb, "null argument");
  XLB_REQUIRE(fa != fb, "f_A and f_B must be different fields");
  if (int rc = check_mix_grid(s, fa, nullptr, fb, nullptr, bc_mask, missing_mask)) return rc;
  const int d = lattice_d(s->lattice);
  if (int rc = check_mix_output(s, "rho_A", rho_a, 1, fa)) return rc;
  if (int rc = check_mix_output(s, "rho_B", rho_b, 1, fa)) return rc;
  if (int rc = check_mix_output(s, "u", u, d, fa)) return rc;
  if (int rc = check_mix_output(s, "force_A", force_a, d, fa)) return rc;
  if (int rc = check_mix_output(s, "force_B", force_b, d, fa)) return rc;
  XLB_HIP(hipSetDevice(s->ctx->device));
  if (int rc = ensure_densities(s, fa)) return rc;
  for (xlbhip_field* o : {rho_a, rho_b, u, force_a, force_b})
    if (o) touch(o);
  MixLaunch q = mix_launch(s, fa, fb, bc_mask, missing_mask, 1.0, 1.0);
  if (int rc = mix_dispatch(s, q, MixKernel::density)) return rc;
  q.out_rho_a = rho_a ? rho_a->data : nullptr;
  q.out_rho_b = rho_b ? rho_b->data : nullptr;
  q.out_u = u ? u->data : nullptr;
  q.out_force_a = force_a ? force_a->data : nullptr;
  q.out_force_b = force_b ? force_b->data : nullptr;
  q.u_stride = u ? u->plane_stride : 0;
  q.force_a_stride = force_a ? force_a->plane_stride : 0;
  q.force_b_stride = force_b ? force_b->plane_stride : 0;
  return mix_dispatch(s, q, MixKernel::out);
}

}  // namespace xlb

extern "C" {

int xlbhip_multicomponent_create(xlbhip_ctx* c, int lattice, int cdt, int sdt, int n_bc, const xlbhip_bc_desc* bcs, xlbhip_multicomponent** out) {
  const auto refusal = [](int kind) {
    return bc_multiphase_accepts(kind) ? nullptr
                                       : "multicomponent: bc kind %d is not supported (resting halfway bounce-back and fullway bounce-back only: the "
                                         "missing directions of other kinds have no neighbour density)";
  };
  const auto own = [&](xlbhip_multicomponent& s) {
    const int q = lattice_q(lattice);
    for (int i = 0; i < n_bc; ++i) {
      XLB_REQUIRE(bcs[i].id != (int)BC_ID_SOLID, "multicomponent: bc id 255 is the solid cells' id");
      for (int l = 0; l < q; ++l)
        XLB_REQUIRE(bcs[i].kind != XLBHIP_BC_HALFWAY_BB || bcs[i].values[l] == 0.0,
                    "multicomponent: the halfway wall of bc id %d has a wall velocity; its constant 6 w (c.u_w) assumes density 1 and would inject the "
                    "wrong momentum into a component of another density",
                    bcs[i].id);
    }
    if (int rc = upload_values(cdt, std::vector<double>(256, 0.0), s.wall_a)) return rc;
    return upload_values(cdt, std::vector<double>(256, 0.0), s.wall_b);
  };
  return create_row_stepper(c, lattice, cdt, sdt, n_bc, bcs, MULTICOMPONENT_POLICY_SUBJECT, refusal, own, out);
}

int xlbhip_multicomponent_destroy(xlbhip_multicomponent* s) { return destroy_drained(s); }

int xlbhip_multicomponent_set_model(xlbhip_multicomponent* s, double g_aa, double g_ab, double g_bb, const double* force) {
  XLB_REQUIRE(s, "null argument");
  XLB_REQUIRE(std::isfinite(g_aa) && std::isfinite(g_ab) && std::isfinite(g_bb), "an interaction strength (G_AA, G_AB, G_BB) is not finite");
  for (int a = 0; a < 3; ++a) XLB_REQUIRE(!force || std::isfinite(force[a]), "the force vector is not finite");
  s->g_aa = g_aa;
  s->g_ab = g_ab;
  s->g_bb = g_bb;
  for (int a = 0; a < 3; ++a) s->force[a] = force ? force[a] : 0.0;
  return 0;
}

int xlbhip_multicomponent_set_wall_density(xlbhip_multicomponent* s, int n, const int32_t* bc_ids, const double* rho_w_a, const double* rho_w_b) {
  XLB_REQUIRE(s && n >= 0 && (n == 0 || (bc_ids && rho_w_a && rho_w_b)), "bad argument");
  std::vector<double> ta(256, 0.0), tb(256, 0.0);
  for (int i = 0; i < n; ++i) {
    const int id = bc_ids[i];
    XLB_REQUIRE(id == (int)BC_ID_SOLID || (id >= 1 && id < 255 && s->bc.kind_host[id] != 0),
                "wall density for bc id %d, which is none of this stepper's boundary conditions (nor 255, the solid cells)", id);
    XLB_REQUIRE(std::isfinite(rho_w_a[i]) && rho_w_a[i] >= 0.0 && std::isfinite(rho_w_b[i]) && rho_w_b[i] >= 0.0,
                "wall densities of bc id %d: not two finite densities >= 0", id);
    ta[id] = rho_w_a[i];
    tb[id] = rho_w_b[i];
  }
  XLB_HIP(hipSetDevice(s->ctx->device));
  XLB_HIP(hipStreamSynchronize(s->ctx->stream));  // (launches may still read the old tables)
  if (int rc = upload_values(s->cdt, ta, s->wall_a)) return rc;
  return upload_values(s->cdt, tb, s->wall_b);
}

int xlbhip_multicomponent_step(xlbhip_multicomponent* s, const xlbhip_field* fa_src, xlbhip_field* fa_dst, const xlbhip_field* fb_src, xlbhip_field* fb_dst,
                               const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega_a, double omega_b, int64_t timestep) {
  (void)timestep;  // (no time-dependent walls in this step)
  if (int rc = check_mix_step(s, fa_src, fa_dst, fb_src, fb_dst, bc_mask, missing_mask, omega_a, omega_b)) return rc;
  return mix_step_once(s, fa_src, fa_dst, fb_src, fb_dst, bc_mask, missing_mask, omega_a, omega_b);
}

int xlbhip_multicomponent_run(xlbhip_multicomponent* s, xlbhip_field* fa_0, xlbhip_field* fa_1, xlbhip_field* fb_0, xlbhip_field* fb_1,
                              const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega_a, double omega_b, int64_t first_timestep,
                              int64_t n_steps, int* result_in_1) {
  (void)first_timestep;
  XLB_REQUIRE(result_in_1 && n_steps >= 0, "bad argument");
  if (int rc = check_mix_step(s, fa_0, fa_1, fb_0, fb_1, bc_mask, missing_mask, omega_a, omega_b)) return rc;
  return run_alternating(n_steps, result_in_1, [&](int64_t, bool odd) {
    return odd ? mix_step_once(s, fa_1, fa_0, fb_1, fb_0, bc_mask, missing_mask, omega_a, omega_b)
               : mix_step_once(s, fa_0, fa_1, fb_0, fb_1, bc_mask, missing_mask, omega_a, omega_b);
  });
}

int xlbhip_multicomponent_densities(xlbhip_multicomponent* s, const xlbhip_field* fa, const xlbhip_field* fb, const xlbhip_field* bc_mask,
                                    const xlbhip_field* missing_mask, xlbhip_field* rho_a, xlbhip_field* rho_b) {
  XLB_REQUIRE(s && fa && fb && rho_a && rho_b, "null argument");
  XLB_REQUIRE(fa != fb && rho_a != rho_b, "f_A and f_B, rho_A and rho_B must be different fields");
  if (int rc = check_mix_grid(s, fa, nullptr, fb, nullptr, bc_mask, missing_mask)) return rc;
  if (int rc = check_mix_output(s, "rho_A", rho_a, 1, fa)) return rc;
  if (int rc = check_mix_output(s, "rho_B", rho_b, 1, fa)) return rc;
  XLB_HIP(hipSetDevice(s->ctx->device));
  touch(rho_a);
  touch(rho_b);
  MixLaunch q = mix_launch(s, fa, fb, bc_mask, missing_mask, 1.0, 1.0);
  q.rho_a = rho_a->data;
  q.rho_b = rho_b->data;
  return mix_dispatch(s, q, MixKernel::density);
}

int xlbhip_multicomponent_force(xlbhip_multicomponent* s, const xlbhip_field* fa, const xlbhip_field* fb, const xlbhip_field* bc_mask,
                                const xlbhip_field* missing_mask, xlbhip_field* force_a, xlbhip_field* force_b) {
  XLB_REQUIRE(force_a && force_b && force_a != force_b, "null argument, or one field for both forces");
  return mix_outputs(s, fa, fb, bc_mask, missing_mask, nullptr, nullptr, nullptr, force_a, force_b);
}

int xlbhip_multicomponent_macroscopic(xlbhip_multicomponent* s, const xlbhip_field* fa, const xlbhip_field* fb, const xlbhip_field* bc_mask,
                                      const xlbhip_field* missing_mask, xlbhip_field* rho_a, xlbhip_field* rho_b, xlbhip_field* u) {
  XLB_REQUIRE(rho_a && rho_b && u && rho_a != rho_b, "null argument, or one field for both densities");
  return mix_outputs(s, fa, fb, bc_mask, missing_mask, rho_a, rho_b, u, nullptr, nullptr);
}

}  // extern "C"
