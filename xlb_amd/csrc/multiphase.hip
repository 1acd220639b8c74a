// libxlbhip: Shan-Chen pseudopotential flow.  The object owns the boundary tables of the step (a BcTables like a stepper's,
// stepper_tables.hpp), the wall pseudopotentials by bc id and the psi field (one value per cell in the compute dtype, allocated at
// first use); a step enqueues k_psi and k_step_multiphase on the context's compute stream, and nothing here waits for the device.
#include <cmath>
#include <vector>

#include "multiphase_launch.hpp"
#include "stepper_tables.hpp"

using namespace xlb;

struct xlbhip_multiphase : RowStepper {
  DeviceBuf psi_wall;  // [256] compute dtype: Psi(rho_w) by bc id
  DeviceBuf psi;       // [psi_cells] compute dtype
  size_t psi_cells = 0;
  int form = PSI_DENSITY;
  double g = 0.0;
  double par[4] = {0, 0, 0, 0};
  double force[3] = {0, 0, 0};
};

namespace xlb {

// the population field f, with f_other (or nullptr) its double-buffering partner, and the masks
static int check_multiphase_grid(const xlbhip_multiphase* s, const xlbhip_field* f, const xlbhip_field* f_other, const xlbhip_field* bcm,
                                 const xlbhip_field* miss) {
  if (int rc = check_row_fields("multiphase", "population fields", lattice_q(s->lattice), s->sdt, {f, f_other}, true)) return rc;
  return check_single_rank_grid("multiphase", "step kernel", s->lattice, s->bc.n_bc, f, bcm, miss);
}

// an output of `card` planes in the compute dtype on f's grid, or nullptr
static int check_multiphase_output(const xlbhip_multiphase* s, const char* name, const xlbhip_field* out, int card, const xlbhip_field* f) {
  if (!out) return 0;
  XLB_REQUIRE(out->dtype == s->cdt && out->card == card && same_grid(out, f) && out->halo == 0,
              "multiphase: %s must be a field of cardinality %d in the compute dtype on f's grid, without ghost planes", name, card);
  return 0;
}

static int ensure_psi(xlbhip_multiphase* s, const xlbhip_field* f) {
  if (s->psi && s->psi_cells == f->cells()) return 0;
  s->psi_cells = 0;
  XLB_HIP(s->psi.alloc(f->cells() * dtype_size(s->cdt)));  // (hipFree of the old one waits for the launches that read it)
  s->psi_cells = f->cells();
  return 0;
}

static MultiphaseLaunch multiphase_launch(const xlbhip_multiphase* s, const xlbhip_field* fs, const xlbhip_field* bcm, const xlbhip_field* miss, double omega) {
  MultiphaseLaunch q = {};
  StepLaunch& p = q.f;
  p = bc_launch(s->ctx, s->bc, s->cdt, s->sdt, bcm, miss, fs);
  p.src = fs->data;
  p.plane_stride = fs->plane_stride;
  p.omega = omega;
  p.vec = 1;
  p.has_bc = s->bc.n_bc > 0 ? 1 : 0;
  q.psi = s->psi.get();
  q.psi_wall = s->psi_wall.get();
  q.form = s->form;
  q.g = s->g;
  for (int k = 0; k < 4; ++k) q.par[k] = s->par[k];
  for (int k = 0; k < 3; ++k) q.force[k] = s->force[k];
  return q;
}

static int multiphase_dispatch(const xlbhip_multiphase* s, const MultiphaseLaunch& q, MultiphaseKernel which) {
  return launch_for_lattice(s->lattice, launch_multiphase_d2q9, launch_multiphase_d3q19, launch_multiphase_d3q27, q, which);
}

// one step f(t) -> f(t + 1): psi of the post-streaming state, then the forced step that reads it
static int multiphase_step_once(xlbhip_multiphase* s, const xlbhip_field* fs, xlbhip_field* fd, const xlbhip_field* bcm, const xlbhip_field* miss, double omega) {
  touch(fd);
  MultiphaseLaunch q = multiphase_launch(s, fs, bcm, miss, omega);
  q.f.dst = fd->data;
  if (int rc = multiphase_dispatch(s, q, MultiphaseKernel::psi)) return rc;
  return multiphase_dispatch(s, q, MultiphaseKernel::step);
}

static int check_multiphase_step(xlbhip_multiphase* s, const xlbhip_field* fa, const xlbhip_field* fb, const xlbhip_field* bcm, const xlbhip_field* miss,
                                 double omega) {
  XLB_REQUIRE(s && fa && fb, "null argument");
  XLB_REQUIRE(fa != fb, "f_0 and f_1 must be different fields (double buffering)");
  if (int rc = check_multiphase_grid(s, fa, fb, bcm, miss)) return rc;
  if (int rc = check_relaxation("omega", omega)) return rc;
  XLB_HIP(hipSetDevice(s->ctx->device));
  return ensure_psi(s, fa);
}

// k_psi into the object's field, then rho, u and / or F of the post-streaming state of f (each output may be nullptr)
static int multiphase_outputs(xlbhip_multiphase* s, const xlbhip_field* f, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, xlbhip_field* rho,
                              xlbhip_field* u, xlbhip_field* force) {
  XLB_REQUIRE(s && f, "null argument");
  if (int rc = check_multiphase_grid(s, f, nullptr, bc_mask, missing_mask)) return rc;
  const int d = lattice_d(s->lattice);
  if (int rc = check_multiphase_output(s, "rho", rho, 1, f)) return rc;
  if (int rc = check_multiphase_output(s, "u", u, d, f)) return rc;
  if (int rc = check_multiphase_output(s, "force", force, d, f)) return rc;
  XLB_HIP(hipSetDevice(s->ctx->device));
  if (int rc = ensure_psi(s, f)) return rc;
  for (xlbhip_field* o : {rho, u, force})
    if (o) touch(o);
  MultiphaseLaunch q = multiphase_launch(s, f, bc_mask, missing_mask, 1.0);
  if (int rc = multiphase_dispatch(s, q, MultiphaseKernel::psi)) return rc;
  q.out_rho = rho ? rho->data : nullptr;
  q.out_u = u ? u->data : nullptr;
  q.out_force = force ? force->data : nullptr;
  q.u_stride = u ? u->plane_stride : 0;
  q.force_stride = force ? force->plane_stride : 0;
  return multiphase_dispatch(s, q, MultiphaseKernel::out);
}

}  // namespace xlb

extern "C" {

int xlbhip_multiphase_create(xlbhip_ctx* c, int lattice, int cdt, int sdt, int n_bc, const xlbhip_bc_desc* bcs, xlbhip_multiphase** out) {
  const auto refusal = [](int kind) {
    return bc_multiphase_accepts(kind) ? nullptr
                                       : "multiphase: bc kind %d is not supported (halfway bounce-back with a constant wall velocity and fullway "
                                         "bounce-back only: the missing directions of other kinds have no neighbour pseudopotential)";
  };
  const auto own = [&](xlbhip_multiphase& s) {
    for (int i = 0; i < n_bc; ++i) XLB_REQUIRE(bcs[i].id != (int)BC_ID_SOLID, "multiphase: bc id 255 is the solid cells' id");
    return upload_values(cdt, std::vector<double>(256, 0.0), s.psi_wall);
  };
  return create_row_stepper(c, lattice, cdt, sdt, n_bc, bcs, MULTIPHASE_POLICY_SUBJECT, refusal, own, out);
}

int xlbhip_multiphase_destroy(xlbhip_multiphase* s) { return destroy_drained(s); }

int xlbhip_multiphase_set_model(xlbhip_multiphase* s, int form, double g, int n_params, const double* params, const double* force) {
  XLB_REQUIRE(s, "null argument");
  XLB_REQUIRE(form == PSI_EXPONENTIAL || form == PSI_DENSITY || form == PSI_CARNAHAN_STARLING, "unknown pseudopotential form %d", form);
  XLB_REQUIRE(n_params >= 0 && n_params <= 4 && (n_params == 0 || params), "a pseudopotential takes up to four parameters (%d given)", n_params);
  XLB_REQUIRE(n_params == (form == PSI_EXPONENTIAL ? 1 : form == PSI_DENSITY ? 0 : 4), "pseudopotential form %d: wrong number of parameters (%d)", form,
              n_params);
  XLB_REQUIRE(std::isfinite(g), "the interaction strength G is not finite");
  XLB_REQUIRE(form != PSI_CARNAHAN_STARLING || g == -1.0, "the Carnahan-Starling form fixes G = -1 (%g given)", g);
  for (int k = 0; k < n_params; ++k) XLB_REQUIRE(std::isfinite(params[k]), "pseudopotential parameter %d is not finite", k);
  XLB_REQUIRE(form != PSI_EXPONENTIAL || params[0] > 0.0, "the exponential form needs rho0 > 0 (%g given)", params[0]);
  s->form = form;
  s->g = g;
  for (int k = 0; k < 4; ++k) s->par[k] = k < n_params ? params[k] : 0.0;
  for (int a = 0; a < 3; ++a) {
    XLB_REQUIRE(!force || std::isfinite(force[a]), "the force vector is not finite");
    s->force[a] = force ? force[a] : 0.0;
  }
  return 0;
}

int xlbhip_multiphase_set_wall_density(xlbhip_multiphase* s, int n, const int32_t* bc_ids, const double* rho_w, const double* psi_w) {
  XLB_REQUIRE(s && n >= 0 && (n == 0 || (bc_ids && rho_w && psi_w)), "bad argument");
  std::vector<double> table(256, 0.0);
  for (int i = 0; i < n; ++i) {
    const int id = bc_ids[i];
    XLB_REQUIRE(id == (int)BC_ID_SOLID || (id >= 1 && id < 255 && s->bc.kind_host[id] != 0),
                "wall density for bc id %d, which is none of this stepper's boundary conditions (nor 255, the solid cells)", id);
    XLB_REQUIRE(std::isfinite(rho_w[i]) && rho_w[i] >= 0.0 && std::isfinite(psi_w[i]), "wall density of bc id %d: not a finite density >= 0", id);
    table[id] = psi_w[i];
  }
  XLB_HIP(hipSetDevice(s->ctx->device));
  XLB_HIP(hipStreamSynchronize(s->ctx->stream));  // (launches may still read the old table)
  return upload_values(s->cdt, table, s->psi_wall);
}

int xlbhip_multiphase_step(xlbhip_multiphase* s, const xlbhip_field* f_src, xlbhip_field* f_dst, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask,
                           double omega, int64_t timestep) {
  (void)timestep;  // (no time-dependent walls in this step)
  if (int rc = check_multiphase_step(s, f_src, f_dst, bc_mask, missing_mask, omega)) return rc;
  return multiphase_step_once(s, f_src, f_dst, bc_mask, missing_mask, omega);
}

int xlbhip_multiphase_run(xlbhip_multiphase* s, xlbhip_field* f_a, xlbhip_field* f_b, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega,
                          int64_t first_timestep, int64_t n_steps, int* result_in_b) {
  (void)first_timestep;
  XLB_REQUIRE(result_in_b && n_steps >= 0, "bad argument");
  if (int rc = check_multiphase_step(s, f_a, f_b, bc_mask, missing_mask, omega)) return rc;
  return run_alternating(n_steps, result_in_b, [&](int64_t, bool odd) {
    return odd ? multiphase_step_once(s, f_b, f_a, bc_mask, missing_mask, omega) : multiphase_step_once(s, f_a, f_b, bc_mask, missing_mask, omega);
  });
}

int xlbhip_multiphase_psi(xlbhip_multiphase* s, const xlbhip_field* f, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, xlbhip_field* psi) {
  XLB_REQUIRE(s && f && psi, "null argument");
  if (int rc = check_multiphase_grid(s, f, nullptr, bc_mask, missing_mask)) return rc;
  if (int rc = check_multiphase_output(s, "psi", psi, 1, f)) return rc;
  XLB_HIP(hipSetDevice(s->ctx->device));
  touch(psi);
  MultiphaseLaunch q = multiphase_launch(s, f, bc_mask, missing_mask, 1.0);
  q.psi = psi->data;
  return multiphase_dispatch(s, q, MultiphaseKernel::psi);
}

int xlbhip_multiphase_force(xlbhip_multiphase* s, const xlbhip_field* f, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, xlbhip_field* force) {
  XLB_REQUIRE(force, "null argument");
  return multiphase_outputs(s, f, bc_mask, missing_mask, nullptr, nullptr, force);
}

int xlbhip_multiphase_macroscopic(xlbhip_multiphase* s, const xlbhip_field* f, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, xlbhip_field* rho,
                                  xlbhip_field* u) {
  XLB_REQUIRE(rho && u, "null argument");
  return multiphase_outputs(s, f, bc_mask, missing_mask, rho, u, nullptr);
}

}  // extern "C"
