// Context of libhfmi.so (include/hfmi.h): error text, version and build tag, the context object with its storage pool,
// workspaces, pinned staging and cached temporaries, status read-backs, timers and the profiler.  Host side only.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <new>

#include "hfmi_eig_plan.h"
#include "hfmi_internal.h"

// ------------------------------------------------------------------ errors
static thread_local char g_err[1024] = "";
void hfmi_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* hfmi_last_error(void) { return g_err; }
extern "C" int hfmi_version(void) { return HFMI_VERSION; }
#ifndef HFMI_BUILD_TAG
#define HFMI_BUILD_TAG "untagged"
#endif
extern "C" const char* hfmi_build_tag(void) { return HFMI_BUILD_TAG; }

extern "C" int hfmi_device_count(int* count) {
  if (!count) HFMI_FAIL(HFMI_ERR_INVALID, "device_count: null argument");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    n = 0;
  }
  *count = n;
  return HFMI_OK;
}

// ------------------------------------------------------------------ device memory: pool of released block storage
// block storage back to the device, once nothing queued on the stream can still use it
static void storage_free(hfmi_ctx* ctx, void* p) {
  (void)hipStreamSynchronize(ctx->stream);
  own_release(OWN_DEVICE, p);
}
static void pool_flush(hfmi_ctx* ctx) {
  if (ctx->pool.empty()) return;
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& e : ctx->pool) own_release(OWN_DEVICE, e.p);
  ctx->pool.clear();
  ctx->pool_bytes = 0;
}
// storage of a destroyed block: kept for reuse (same stream order as every other use of it) or freed
void pool_release(hfmi_ctx* ctx, void* p, size_t bytes) {
  constexpr size_t MAX_ENTRY = (size_t)2 << 30, MAX_TOTAL = (size_t)8 << 30;
  if (bytes <= MAX_ENTRY && ctx->pool.size() < 16 && ctx->pool_bytes + bytes <= MAX_TOTAL) {
    ctx->pool.push_back({p, bytes});
    ctx->pool_bytes += bytes;
    return;
  }
  storage_free(ctx, p);
}
static void* pool_take(hfmi_ctx* ctx, size_t bytes) {
  for (size_t i = ctx->pool.size(); i-- > 0;)
    if (ctx->pool[i].bytes == bytes) {
      void* p = ctx->pool[i].p;
      ctx->pool_bytes -= bytes;
      ctx->pool.erase(ctx->pool.begin() + i);
      return p;
    }
  return nullptr;
}

int block_alloc(hfmi_ctx* ctx, int64_t N, int nvec, hfmi_block** out) {
  if (N <= 0 || nvec <= 0) HFMI_FAIL(HFMI_ERR_INVALID, "block: N=%lld nvec=%d must be positive", (long long)N, nvec);
  hfmi_block* b = new (std::nothrow) hfmi_block();
  if (!b) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  b->ctx = ctx;
  b->N = N;
  b->nvec = nvec;
  b->ld = round_up(N, 32);
  b->owner = true;
  const size_t bytes = (size_t)b->ld * nvec * sizeof(double);
  b->p = (double*)pool_take(ctx, bytes);
  hipError_t e = b->p ? hipSuccess : (hipError_t)own_acquire(OWN_DEVICE, bytes, (void**)&b->p);
  if (e != hipSuccess && !ctx->pool.empty()) {      // give the pooled storage back and try once more
    pool_flush(ctx);
    e = (hipError_t)own_acquire(OWN_DEVICE, bytes, (void**)&b->p);
  }
  if (e != hipSuccess) {
    const double gb = (double)b->ld * nvec * 8 / 1e9;
    delete b;
    HFMI_FAIL(HFMI_ERR_HIP, "hipMalloc of a %lld x %d block (%.2f GB) failed: %s", (long long)N, nvec, gb, hipGetErrorString(e));
  }
  *out = b;
  return HFMI_OK;
}

void ctx_watch_comm(hfmi_ctx* ctx, hfmi_comm* c) {
  if (ctx && c) ctx->watched_comms.push_back(c);
}
void ctx_unwatch_comm(hfmi_ctx* ctx, hfmi_comm* c) {
  if (!ctx) return;
  for (size_t i = 0; i < ctx->watched_comms.size(); ++i)
    if (ctx->watched_comms[i] == c) {
      ctx->watched_comms.erase(ctx->watched_comms.begin() + i);
      return;
    }
}
// after a host synchronisation: did a stream-ordered collective behind it give up?  (one read of pinned host memory per
// communicator; no device call)
int ctx_check_comm(hfmi_ctx* ctx) {
  for (hfmi_comm* c : ctx->watched_comms) HFMI_TRY(comm_check_error(c));
  return HFMI_OK;
}

int ctx_ws(hfmi_ctx* ctx, int slot, size_t bytes, void** out) {
  auto& buf = ctx->ws[slot];
  const auto drain = [&]() -> int {
    hipError_t e = hipStreamSynchronize(ctx->stream);
    // buffers other streams work in: the panel reductions' staging area (auxiliary stream), the ingest buffer
    if (e == hipSuccess && slot == WS_COMM) e = hipStreamSynchronize(ctx->aux_stream);
    if (e == hipSuccess && slot == WS_INGEST) e = hipStreamSynchronize(ctx->ingest_stream);
    return (int)e;
  };
  const size_t slack = bytes / 4 + 4096;
  int e = grow(buf, bytes, drain, slack);
  if (e != 0 && !ctx->pool.empty()) {      // give the pooled storage back and try once more
    pool_flush(ctx);
    e = grow(buf, bytes, drain, slack);
  }
  OWN_TRY(e);
  *out = buf.get();
  return HFMI_OK;
}
int ctx_pinned(hfmi_ctx* ctx, size_t bytes, void** out) {
  OWN_TRY(grow(ctx->pinned, bytes, [&] { return (int)hipStreamSynchronize(ctx->stream); }));
  *out = ctx->pinned.get();
  return HFMI_OK;
}

// ------------------------------------------------------------------ context
extern "C" int hfmi_ctx_create(int device, hfmi_ctx** out) {
  if (!out) HFMI_FAIL(HFMI_ERR_INVALID, "ctx_create: null out");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    HFMI_FAIL(HFMI_ERR_NO_DEVICE, "no HIP device visible (libhfmi has no CPU path)");
  }
  if (device < 0 || device >= n) HFMI_FAIL(HFMI_ERR_INVALID, "ctx_create: device %d out of range [0,%d)", device, n);
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  std::unique_ptr<hfmi_ctx> c(new (std::nothrow) hfmi_ctx());
  if (!c) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  c->device = device;
  c->num_cus = prop.multiProcessorCount;
  c->lds_per_block = prop.sharedMemPerBlock;
  OWN_TRY(c->stream.create(hipStreamNonBlocking));
  OWN_TRY(c->ev0.create());
  OWN_TRY(c->ev1.create());
  OWN_TRY(c->aux_stream.create(hipStreamNonBlocking));
  OWN_TRY(c->ev_status.create(hipEventDisableTiming));
  OWN_TRY(c->ev_side.create(hipEventDisableTiming));
  for (hip_event& e : c->ev_cb) OWN_TRY(e.create(hipEventDisableTiming));
  for (hip_event& e : c->ev_panel) OWN_TRY(e.create(hipEventDisableTiming));
  OWN_TRY(c->ev_join.create(hipEventDisableTiming));
  OWN_TRY(c->small.alloc((size_t)SM_NSLOTS * SM_MAXK * SM_LD));
  HIP_TRY(hipMemsetAsync(c->small, 0, c->small.bytes(), c->stream));
  OWN_TRY(c->status_words.alloc(2));
  c->status_dev = c->status_words;
  HIP_TRY(hipMemsetAsync(c->status_dev, 0, c->status_words.bytes(), c->stream));
  OWN_TRY(c->status_host.alloc(1));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *out = c.release();
  return HFMI_OK;
}

// What a kernel may still use is released only after the streams have drained; the members then go in reverse order of their
// declaration, the streams last.
hfmi_ctx::~hfmi_ctx() {
  (void)hipSetDevice(device);
  if (stream) (void)hipStreamSynchronize(stream);
  if (aux_stream) (void)hipStreamSynchronize(aux_stream);
  if (ingest_stream) (void)hipStreamSynchronize(ingest_stream);
  for (hfmi_comm* c : watched_comms) comm_forget_ctx(c);    // a communicator destroyed after its context must not look for it
  for (hfmi_block* b : tmp_blocks)
    if (b) {
      if (b->owner && b->p) own_release(OWN_DEVICE, b->p);
      delete b;
    }
  for (auto& e : pool) own_release(OWN_DEVICE, e.p);
  xfer_destroy(this);
}
extern "C" int hfmi_ctx_destroy(hfmi_ctx* ctx) {
  delete ctx;
  return HFMI_OK;
}

extern "C" int hfmi_plan_clear(hfmi_ctx* ctx) {
  if (!ctx) HFMI_FAIL(HFMI_ERR_INVALID, "null ctx");
  ctx->plan_count = 0;
  return HFMI_OK;
}
extern "C" int hfmi_plan_read(hfmi_ctx* ctx, int max_records, int* words, int* nrecords, int* total) {
  if (!ctx || !nrecords || (max_records > 0 && !words)) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  int64_t n = ctx->plan_count < HFMI_PLAN_RING ? ctx->plan_count : HFMI_PLAN_RING;
  if (n > max_records) n = max_records < 0 ? 0 : max_records;
  const int64_t first = ctx->plan_count - n;     // the n newest, oldest first
  for (int64_t i = 0; i < n; ++i)
    memcpy(words + i * HFMI_PLAN_WORDS, ctx->plan_ring[(first + i) % HFMI_PLAN_RING], sizeof(int) * HFMI_PLAN_WORDS);
  *nrecords = (int)n;
  if (total) *total = (int)(ctx->plan_count > 0x7fffffff ? 0x7fffffff : ctx->plan_count);
  return HFMI_OK;
}

// the records a launch of that shape would append, from the planners the launchers call (hfmi_tsgemm_plan.h); no device involved
extern "C" int hfmi_plan_predict(int kind, int m, int k, int64_t N, double scale, double beta, int64_t rs, int64_t cs, int nsplit_req,
                                 int flags, int num_cus, int hook_panels, int max_records, int* words, int64_t* hook_rows, int* nrecords) {
  if (!nrecords || (max_records > 0 && !words)) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (m <= 0 || k <= 0 || N <= 0 || hook_panels < 0 || hook_panels > NN_MAX_PANELS) HFMI_FAIL(HFMI_ERR_INVALID, "plan_predict: bad shape");
  const tsgemm_knobs& kn = tsgemm_knobs_ref();
  int n = 0, spill[HFMI_PLAN_WORDS];
  auto slot = [&](int64_t row0, int64_t rows) {
    const bool fits = n < max_records;
    if (fits && hook_rows) hook_rows[2 * n] = row0, hook_rows[2 * n + 1] = rows;
    return fits ? words + (size_t)HFMI_PLAN_WORDS * n++ : (++n, spill);
  };
  auto reduce = [&](const reduce_call& c) { reduce_plan_words(reduce_plan_make(c, rs, cs, !(flags & HFMI_PREDICT_UNALIGNED)), slot(0, 0)); };
  if (kind == HFMI_PREDICT_TN) {
    for (int k0 = 0; k0 < k; k0 += 256) {
      const tn_plan p = tn_plan_make(m, k - k0 < 256 ? k - k0 : 256, N, scale, beta, rs, cs, flags & HFMI_PREDICT_ALIASED, nsplit_req, kn, num_cus);
      if (!p.has_instance) HFMI_FAIL(HFMI_ERR_INVALID, "tsgemm_tn: no instance for MT=%d NT=%d WAVES=%d", p.mt, p.nt, p.waves);
      tn_plan_words(p, slot(0, 0));
      for (int i = 0; i < p.nred; ++i) reduce(p.red[i]);
    }
  } else if (kind == HFMI_PREDICT_SS) {
    const bool same = flags & HFMI_PREDICT_SAME;
    if (!ss_applicable(m, k, same)) HFMI_FAIL(HFMI_ERR_INVALID, "plan_predict: not a skinny x skinny shape");
    const ss_plan p = ss_plan_make(m, k, N, same, nsplit_req, kn, num_cus);
    if (!p.has_instance) HFMI_FAIL(HFMI_ERR_INVALID, "tsgemm_ss: no instance for tiles/wave=%d chunks/thread=%d", p.tpw, p.nq);
    ss_plan_words(p, slot(0, 0));
    reduce(p.red);
  } else if (kind == HFMI_PREDICT_NN) {
    for (int r0 = 0; r0 < k; r0 += 256) {
      const int rp = k - r0 < 256 ? k - r0 : 256;
      const nn_plan p = nn_plan_make(m, rp, N, flags & HFMI_PREDICT_UPPER, hook_panels, kn, num_cus);
      if (!p.has_instance) HFMI_FAIL(HFMI_ERR_INVALID, "tsgemm_nn: panel too wide (%d)", rp);
      if (p.res) nn_res_plan_words(p, slot(0, 0));
      for (int i = 0; i < p.nlaunch; ++i) nn_launch_words(p, p.launch[i], slot(p.launch[i].hook_row0, p.launch[i].hook_rows));
    }
  } else {
    HFMI_FAIL(HFMI_ERR_INVALID, "plan_predict: unknown kind %d", kind);
  }
  *nrecords = n;
  if (n > max_records) HFMI_FAIL(HFMI_ERR_INVALID, "plan_predict: %d records, room for %d", n, max_records);
  return HFMI_OK;
}

// the plan of the whole-GPU eigensolver for n, from the planner and the walk the driver runs (hfmi_eig_plan.h); no device involved
static_assert(EIG_NREGIONS == HFMI_EIG_PLAN_REGIONS && EIG_NINST == HFMI_EIG_PLAN_INSTANCES && EB_MAX_LEVELS == HFMI_EIG_PLAN_LEVELS,
              "include/hfmi.h sizes the outputs of hfmi_eig_plan_predict");
extern "C" int hfmi_eig_plan_predict(int n, int nvec, int64_t lds_per_block, int64_t defl1_static_lds, int64_t* scalars, int64_t* regions,
                                     int64_t* levels, int64_t* walk) {
  if (!scalars || !regions || !levels || !walk) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (n < 1 || n > EB_MAXN || lds_per_block < 0 || defl1_static_lds < 0) HFMI_FAIL(HFMI_ERR_INVALID, "eig_plan_predict: bad argument");
  if (nvec < 0 || nvec > n) nvec = n;
  const eig_knobs& kn = eig_knobs_ref();
  const eig_plan p = eig_plan_make(n, nvec, kn, (size_t)lds_per_block, (size_t)defl1_static_lds);
  memset(scalars, 0, sizeof(int64_t) * HFMI_EIG_PLAN_SCALARS);
  memset(regions, 0, sizeof(int64_t) * 4 * HFMI_EIG_PLAN_REGIONS);
  memset(levels, 0, sizeof(int64_t) * 4 * HFMI_EIG_PLAN_LEVELS);
  memset(walk, 0, sizeof(int64_t) * 4 * HFMI_EIG_PLAN_INSTANCES);
  scalars[0] = p.blocked;
  if (!p.blocked) return HFMI_OK;
  eig_walk_summary w;
  (void)eig_tri_walk(p, w);
  const int64_t sc[HFMI_EIG_PLAN_SCALARS] = {1, p.nr, p.ld, p.npad, p.WY, p.nblk, p.npanels, p.Lf, (int64_t)p.vlen, (int64_t)p.bytes,
                                             p.tri_b_lds_attr, w.j_unb, w.panel_cols, w.panel_ends, w.mirrors, w.lower_updates, w.tails,
                                             w.max_ntiles, w.max_npvy_all, w.max_nb, w.max_ga, kn.sym_min, kn.unb_max, kn.leaf_max};
  memcpy(scalars, sc, sizeof(sc));
  for (int i = 0; i < EIG_NREGIONS; ++i) {
    const eig_region& r = p.region[i];
    const int64_t v[4] = {r.elem, (int64_t)r.count, (int64_t)r.offset, (int64_t)r.bytes()};
    memcpy(regions + 4 * i, v, sizeof(v));
  }
  for (int L = 0; L < p.Lf; ++L) {
    const int64_t v[4] = {p.level[L].cap, p.level[L].mode, p.level[L].lds, p.level[L].raise};
    memcpy(levels + 4 * L, v, sizeof(v));
  }
  for (int i = 0; i < EIG_NINST; ++i) {
    const int64_t v[4] = {w.launches[i], w.max_npn[i], w.max_npvy[i], w.max_lds[i]};
    memcpy(walk + 4 * i, v, sizeof(v));
  }
  return HFMI_OK;
}

// the launch plan of a call of the one-workgroup k x k stage, from the planner its launcher asks (hfmi_small_plan.h); no device involved
static_assert(SMALL_KNOB_WORDS == HFMI_SMALL_KNOB_WORDS && SMALL_PLAN_WORDS == HFMI_SMALL_PLAN_WORDS,
              "include/hfmi.h sizes the arrays of hfmi_small_plan_predict");
extern "C" int hfmi_small_plan_predict(int kind, int k, int method, const int* knobs, int64_t* words) {
  if (!words) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  const small_knobs kn = knobs ? small_knobs_from_words(knobs) : small_knobs_ref();
  small_plan p;
  switch (kind) {
    case SMALL_KIND_CHOL: p = chol_plan(k, kn); break;
    case SMALL_KIND_EIGH: p = sym_eig_route(method, kn) ? jacobi_eig_plan(k, kn) : dc_eig_plan(k, kn); break;
    case SMALL_KIND_SVD: p = jacobi_svd_plan(k, kn); break;
    case SMALL_KIND_LU: p = lu_plan(k); break;
    default: HFMI_FAIL(HFMI_ERR_INVALID, "small_plan_predict: unknown kind %d", kind);
  }
  small_plan_words(p, kn, words);
  return HFMI_OK;
}

// the rules of the sparse SPD solves, from the functions cheb_solve, amg_smooth and launch_cheb_step ask (hfmi_spsolve_rules.h)
static_assert(CHEB_RULES_WORDS == HFMI_CHEB_RULES_WORDS, "include/hfmi.h sizes the array of hfmi_cheb_rules_predict");
extern "C" int hfmi_cheb_rules_predict(double lmin, double lmax, double rel_tol, int max_iter, int64_t nrows, int k, int resid, const int* knobs,
                                       int nsteps, double* coef, int64_t* words) {
  if (!words || (nsteps > 0 && !coef)) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (!(lmin > 0.0) || !(lmax >= lmin) || nrows < 1 || k < 1 || nsteps < 0) HFMI_FAIL(HFMI_ERR_INVALID, "cheb_rules_predict: bad argument");
  const spsolve_knobs kn = knobs ? spsolve_knobs_make(knobs[0], knobs[1], knobs[2]) : spsolve_knobs_ref();
  cheb_rules_words(cheb_solve_plan(lmin, lmax, rel_tol, max_iter), cheb_step_plan(nrows, k, resid != 0, kn), kn, words);
  cheb_recurrence rec(lmin, lmax);
  if (coef) {
    coef[0] = rec.inv_theta();
    coef[1] = rec.spread() ? 1.0 : 0.0;
    for (int i = 0; i < nsteps && rec.spread(); ++i) rec.next(coef + 2 + 2 * i, coef + 3 + 2 * i);
  }
  return HFMI_OK;
}
extern "C" int hfmi_lanczos_bracket_predict(int m, const double* rz, const double* pap, double gersh_lmax, int* refusal, double* values) {
  if (!refusal || !values || (m > 0 && (!rz || !pap)) || m < 0) HFMI_FAIL(HFMI_ERR_INVALID, "lanczos_bracket_predict: bad argument");
  lanczos_run run;
  bool spd = true;
  for (int i = 0; i < m && spd; ++i) spd = run.push(rz[i], pap[i], rz[i + 1]);
  cheb_bracket br = lanczos_bracket(run.alpha, run.beta, gersh_lmax);
  if (!spd && br.refusal != LANCZOS_NO_GERSHGORIN) br = cheb_bracket{LANCZOS_NOT_SPD, 0.0, 0.0, 0.0, 0.0};   // cheb_estimate's order
  *refusal = br.refusal;
  const double v[4] = {br.tmin, br.tmax, br.lmin, br.lmax};
  memcpy(values, v, sizeof(v));
  return HFMI_OK;
}

// the launch plan of the FFT apply of a kernel covariance on a grid, from the planner fftcov_apply asks (hfmi_fftcov_plan.h)
static_assert(FFTCOV_PLAN_WORDS == HFMI_FFTCOV_PLAN_WORDS, "include/hfmi.h sizes the array of hfmi_fftcov_plan_predict");
extern "C" int hfmi_fftcov_plan_predict(int d, const int64_t* n, int nvec, int64_t budget_bytes, int64_t* words) {
  if (!n || !words) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (d < 1 || d > 3) HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_plan_predict: d = %d is not 1, 2 or 3", d);
  for (int c = 0; c < d; ++c)
    if (n[c] < 1 || n[c] > FFTCOV_MAXN) HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_plan_predict: n[%d] = %lld is not in 1 .. %d", c, (long long)n[c], FFTCOV_MAXN);
  if (nvec < 0) HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_plan_predict: negative number of vectors");
  fftcov_plan p = fftcov_plan_passes(d, n, false);
  fftcov_plan_chunks(p, nvec, budget_bytes, fftcov_pairs_knob());
  fftcov_plan_words(p, words);
  return HFMI_OK;
}

// ... and of a draw of the grid sampler at growth `growth` (hfmi_grid_sampler_draw asks the same planner)
extern "C" int hfmi_fftcov_sample_plan_predict(int d, const int64_t* n, int growth, int nsamples, int64_t budget_bytes, int64_t* words) {
  if (!n || !words) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (d < 1 || d > 3) HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_sample_plan_predict: d = %d is not 1, 2 or 3", d);
  for (int c = 0; c < d; ++c)
    if (n[c] < 1 || n[c] > FFTCOV_MAXN) HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_sample_plan_predict: n[%d] = %lld is not in 1 .. %d", c, (long long)n[c], FFTCOV_MAXN);
  if (nsamples < 0) HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_sample_plan_predict: negative number of draws");
  if (!fftcov_growth_feasible(d, n, growth))
    HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_sample_plan_predict: growth %d is outside 0..%d or takes an axis past %d entries", growth, FFTCOV_MAX_GROWTH, FFTCOV_MAXP);
  fftcov_plan p = fftcov_sample_plan_passes(d, n, growth, false);
  fftcov_plan_chunks(p, nsamples, budget_bytes, fftcov_pairs_knob());
  fftcov_sample_plan_words(p, growth, words);
  return HFMI_OK;
}
// ... and of an apply of the factor S (transpose 0) or S^T (1) of that embedding (hfmi_op_grid_factor asks the same planner)
extern "C" int hfmi_fftcov_factor_plan_predict(int d, const int64_t* n, int growth, int transpose, int nvec, int64_t budget_bytes, int64_t* words) {
  if (!n || !words) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (d < 1 || d > 3) HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_factor_plan_predict: d = %d is not 1, 2 or 3", d);
  for (int c = 0; c < d; ++c)
    if (n[c] < 1 || n[c] > FFTCOV_MAXN) HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_factor_plan_predict: n[%d] = %lld is not in 1 .. %d", c, (long long)n[c], FFTCOV_MAXN);
  if (nvec < 0) HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_factor_plan_predict: negative number of vectors");
  if (transpose != 0 && transpose != 1) HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_factor_plan_predict: transpose = %d is not 0 or 1", transpose);
  if (!fftcov_growth_feasible(d, n, growth))
    HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_factor_plan_predict: growth %d is outside 0..%d or takes an axis past %d entries", growth, FFTCOV_MAX_GROWTH, FFTCOV_MAXP);
  fftcov_plan p = fftcov_factor_plan_passes(d, n, growth, transpose);
  fftcov_plan_chunks(p, nvec, budget_bytes, fftcov_pairs_knob());
  fftcov_factor_plan_words(p, growth, transpose, words);
  return HFMI_OK;
}
// ... and of the long route (split-line passes): kind 0 apply (growth 0), 1 draw, 2 factor S, 3 factor S^T, at that longest line
static_assert(FFTCOV_LONG_PLAN_WORDS == HFMI_FFTCOV_LONG_PLAN_WORDS, "include/hfmi.h sizes the array of hfmi_fftcov_long_plan_predict");
extern "C" int hfmi_fftcov_long_plan_predict(int kind, int d, const int64_t* n, int growth, int max_line, int nvec, int64_t budget_bytes,
                                             int64_t* words) {
  if (!n || !words) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (kind < FFTCOV_KIND_APPLY || kind > FFTCOV_KIND_FACTOR_T) HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_long_plan_predict: kind %d is not 0 .. 3", kind);
  if (d < 1 || d > 3) HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_long_plan_predict: d = %d is not 1, 2 or 3", d);
  for (int c = 0; c < d; ++c)
    if (n[c] < 1 || n[c] > FFTCOV_LONG_MAXN)
      HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_long_plan_predict: n[%d] = %lld is not in 1 .. %lld", c, (long long)n[c], (long long)FFTCOV_LONG_MAXN);
  if (nvec < 0) HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_long_plan_predict: negative number of vectors");
  if (!fftcov_max_line_ok(max_line))
    HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_long_plan_predict: max_line = %d is not a power of two in %d .. %d", max_line, FFTCOV_LONG_MIN_LINE, FFTCOV_LONG_MAX_LINE);
  if (kind == FFTCOV_KIND_APPLY && growth != 0) HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_long_plan_predict: an apply has growth 0, got %d", growth);
  if (!fftcov_long_feasible(d, n, growth, max_line))
    HFMI_FAIL(HFMI_ERR_INVALID, "fftcov_long_plan_predict: growth %d is outside 0..%d or takes an axis past max_line^2 = %lld entries", growth,
              FFTCOV_LONG_MAX_GROWTH, (long long)max_line * max_line);
  fftcov_long_plan p = fftcov_long_plan_passes(kind, d, n, growth, max_line);
  fftcov_plan_chunks(p.base, nvec, budget_bytes, fftcov_pairs_knob());
  fftcov_long_plan_words(p, growth, kind, words);
  return HFMI_OK;
}

extern "C" int hfmi_ctx_set_stream(hfmi_ctx* ctx, void* hip_stream) {
  if (!ctx) HFMI_FAIL(HFMI_ERR_INVALID, "null ctx");
  if (hip_stream != nullptr && ctx->stream == (hipStream_t)hip_stream) return HFMI_OK;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (hip_stream == nullptr) {
    if (!ctx->stream.owned()) {
      decltype(ctx->stream) own;      // the caller's stream stays in place when this fails
      OWN_TRY(own.create(hipStreamNonBlocking));
      ctx->stream = std::move(own);
    }
  } else {
    ctx->stream.borrow((hipStream_t)hip_stream);
  }
  return HFMI_OK;
}
extern "C" int hfmi_ctx_get_stream(hfmi_ctx* ctx, void** hip_stream) {
  if (!ctx || !hip_stream) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  *hip_stream = (void*)ctx->stream;
  return HFMI_OK;
}
extern "C" int hfmi_ctx_synchronize(hfmi_ctx* ctx) {
  if (!ctx) HFMI_FAIL(HFMI_ERR_INVALID, "null ctx");
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return ctx_check_comm(ctx);
}
extern "C" int hfmi_ctx_device_info(hfmi_ctx* ctx, char* name, int name_len, int* compute_units, int64_t* hbm_bytes) {
  if (!ctx) HFMI_FAIL(HFMI_ERR_INVALID, "null ctx");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
  if (name && name_len > 0) {
    snprintf(name, name_len, "%s (%s)", prop.name, prop.gcnArchName);
  }
  if (compute_units) *compute_units = prop.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
  return HFMI_OK;
}
extern "C" int hfmi_ctx_pci_bus_id(hfmi_ctx* ctx, char* buf, int len) {
  if (!ctx || !buf || len < 16) HFMI_FAIL(HFMI_ERR_INVALID, "ctx_pci_bus_id: bad argument");
  HIP_TRY(hipDeviceGetPCIBusId(buf, len, ctx->device));
  return HFMI_OK;
}
extern "C" int hfmi_timer_start(hfmi_ctx* ctx) {
  if (!ctx) HFMI_FAIL(HFMI_ERR_INVALID, "null ctx");
  HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  return HFMI_OK;
}
extern "C" int hfmi_timer_stop(hfmi_ctx* ctx, double* milliseconds) {
  if (!ctx || !milliseconds) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(hipEventSynchronize(ctx->ev1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *milliseconds = ms;
  return HFMI_OK;
}

// ------------------------------------------------------------------ cached temporaries (enum hfmi_tmp_slot)
// *out: a view of exactly nvec vectors of the slot's cached block (which may hold more and is regrown when it holds fewer)
int ctx_tmp_view(hfmi_ctx* ctx, int idx, int64_t N, int nvec, hfmi_block* out) {
  if ((int)ctx->tmp_blocks.size() <= idx) ctx->tmp_blocks.resize(idx + 1, nullptr);
  hfmi_block* b = ctx->tmp_blocks[idx];
  if (b && (b->N != N || b->nvec < nvec)) {
    storage_free(ctx, b->p);
    delete b;
    b = nullptr;
    ctx->tmp_blocks[idx] = nullptr;
  }
  if (!b) {
    HFMI_TRY(block_alloc(ctx, N, nvec, &b));
    HIP_TRY(hipMemsetAsync(b->p, 0, (size_t)b->ld * nvec * sizeof(double), ctx->stream));
    ctx->tmp_blocks[idx] = b;
  }
  *out = *b;
  out->nvec = nvec;
  out->owner = false;
  return HFMI_OK;
}

// read `count` doubles of device memory back to the host (synchronises the stream)
int read_back(hfmi_ctx* ctx, const double* dev, size_t count, double* host) {
  void* pin = nullptr;
  HFMI_TRY(ctx_pinned(ctx, count * sizeof(double), &pin));
  HIP_TRY(hipMemcpyAsync(pin, dev, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HFMI_TRY(ctx_check_comm(ctx));            // what was read may have come through a collective that gave up
  memcpy(host, pin, count * sizeof(double));
  return HFMI_OK;
}
void print_status_dbg(const hfmi_status_words* out) {
  static const bool dbg = env_flag("HFMI_DEBUG_TIMING");
  if (dbg)
    fprintf(stderr, "[hfmi timing] %s cycles: %lld %lld %lld %lld\n",
            out->tick[4] == 3 ? "chol-polish(load,-,-,out)" : out->tick[4] ? "jacobi(total,phase1,phase2,sweeps)" : "chol(load,chol,inv,out)",
            out->tick[0], out->tick[1], out->tick[2], out->tick[3]);
  if (dbg && (!out->tick[4] || out->tick[4] == 3))
    fprintf(stderr, "[hfmi timing]   chol status: min pivot ratio %.3e, input defect %.3e, shifted %d; blocked phases (diag, row, trailing) %lld %lld %lld\n",
            out->min_pivot_ratio, out->gram_dev, out->shifted, out->tick[5], out->tick[6], out->tick[7]);
}
int read_status(hfmi_ctx* ctx, hfmi_status_words* out) {
  HIP_TRY(hipMemcpyAsync(ctx->status_host, ctx->status_dev, sizeof(hfmi_status_words), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  *out = *ctx->status_host;
  print_status_dbg(out);
  return HFMI_OK;
}
// Small device -> host copies that nothing on the main stream waits for: a copy engine / blit between two dependent kernels costs
// the main stream 5 us of copy and 10-15 us of bubbles (timeline of the shard step), on the auxiliary stream it costs nothing.
// side_copies_begin orders the auxiliary stream behind the current point of the main stream; the copies are then enqueued on
// ctx->aux_stream by the caller; side_copies_end leaves an event the main stream can be made to wait for before a kernel
// overwrites the source.
int side_copies_begin(hfmi_ctx* ctx) {
  HIP_TRY(hipEventRecord(ctx->ev_status, ctx->stream));
  HIP_TRY(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_status, 0));
  return HFMI_OK;
}
int side_copies_end(hfmi_ctx* ctx) {
  HIP_TRY(hipEventRecord(ctx->ev_side, ctx->aux_stream));
  return HFMI_OK;
}

int g_comm_panels = -1;    // HFMI_COMM_PANELS: 0 = one all-reduce after the product, n = at most n row panels (default 4)
// What a profiling region (hfmi_profile_begin .. _end) records.  Every record is a pair of events on the stream, and an event
// between two dependent kernels costs 2-4 us of idle GPU: with one pair per contraction and per phase a 64-sample shard step of
// config 4 carried ~32 of them.  Level 2 (default): contractions and phases.  Level 1: only contractions of at least
// HFMI_PROF_MIN_GFLOP (2.0) Gflop -- what a roofline line needs -- and no phases.  Level 3: level 2 plus every launch of a pass of
// the grid kernel covariance (prof_start_pass; measurements of single passes only: an event pair per pass).
static int g_prof_level = 2;
// HFMI_QR_TRUST_FIRST=0 / tuning key "qr_trust_first": the first Cholesky-QR pass of the Gram-form solve waits for its status words
// (the behaviour up to round 4: one host round trip in the middle of every solve); default 1
int g_qr_trust_first = -1;
// tuning key "qr_wide_min": the width from which hfmi_borth_qr takes the wide Cholesky-QR (hfmi_qr.hip); below 257 only so that the
// wide route can be compared with the narrow one at widths both serve
int g_qr_wide_min = SM_MAXK + 1;
int api_tuning_set(const char* key, int value) {
  if (key && !strcmp(key, "comm_panels") && value >= 0 && value <= 8) {
    g_comm_panels = value;
    return 1;
  }
  if (key && !strcmp(key, "prof_level") && value >= 1 && value <= 3) {
    g_prof_level = value;
    return 1;
  }
  if (key && !strcmp(key, "qr_trust_first") && (value == 0 || value == 1)) {
    g_qr_trust_first = value;
    return 1;
  }
  if (key && !strcmp(key, "qr_wide_min") && value >= 17 && value <= SM_MAXK + 1) {
    g_qr_wide_min = value;
    return 1;
  }
  return 0;
}
// Tuning knobs (A/B measurements): the contractions' live in tsgemm_knobs (hfmi_tsgemm_plan.h), the k x k stage's in small_knobs
// (hfmi_small_plan.h), the other subsystems keep their own
extern "C" int hfmi_tuning_set(const char* key, int value) {
  if (key && tsgemm_knob_set(key, value)) {}
  else if (key && small_knob_set(key, value)) {}
  else if (key && api_tuning_set(key, value)) {}
  else if (key && pchol_tuning_set(key, value)) {}
  else if (key && fftcov_knob_set(key, value)) {}
  else if (key && fftcov_sample_knob_set(key, value)) {}
  else if (key && fftcov_long_knob_set(key, value)) {}
  else HFMI_FAIL(HFMI_ERR_INVALID, "tuning_set: unknown key/value");
  return HFMI_OK;
}

// ------------------------------------------------------------------ instrumentation
int prof_start(hfmi_ctx* ctx, int kind, int64_t m, int64_t k, int64_t N) {
  if (!ctx->profiling) return -1;
  if (g_prof_level < 2 && 2.0 * (double)N * (double)m * (double)k < 2.0e9) return -1;
  hfmi_ctx::prof_rec r;
  r.kind = kind;
  r.m = m;
  r.k = k;
  r.N = N;
  // algorithmic work (each operand touched once): flops 2 N m k, bytes 8 (N m + N k + m k)
  r.flops = 2.0 * (double)N * (double)m * (double)k;
  r.bytes = 8.0 * ((double)N * m + (double)N * k + (double)m * k);
  if (r.e0.create() != 0 || r.e1.create() != 0) return -1;
  (void)hipEventRecord(r.e0, ctx->stream);
  ctx->prof.push_back(std::move(r));
  return (int)ctx->prof.size() - 1;
}
// one pass of the grid kernel covariance (kind HFMI_PROF_FFTCOV_PASS, level 3 only): the group is (line length, flags and part,
// index of the pass in its plan), the bytes those the pass moves
int prof_start_pass(hfmi_ctx* ctx, int64_t L, int64_t flags_part, int64_t index, double bytes) {
  if (!ctx->profiling || g_prof_level < 3) return -1;
  hfmi_ctx::prof_rec r;
  r.kind = 2;
  r.m = L;
  r.k = flags_part;
  r.N = index;
  r.flops = 0.0;
  r.bytes = bytes;
  if (r.e0.create() != 0 || r.e1.create() != 0) return -1;
  (void)hipEventRecord(r.e0, ctx->stream);
  ctx->prof.push_back(std::move(r));
  return (int)ctx->prof.size() - 1;
}
int prof_stop(hfmi_ctx* ctx, int idx) {
  if (idx >= 0) (void)hipEventRecord(ctx->prof[idx].e1, ctx->stream);
  return HFMI_OK;
}
int phase_begin_on(hfmi_ctx* ctx, int phase, hipStream_t st) {
  if (!ctx->profiling || g_prof_level < 2) return -1;
  hfmi_ctx::phase_rec r;
  r.phase = phase;
  if (r.e0.create() != 0 || r.e1.create() != 0) return -1;
  (void)hipEventRecord(r.e0, st);
  ctx->phase_events.push_back(std::move(r));
  return (int)ctx->phase_events.size() - 1;
}
void phase_end_on(hfmi_ctx* ctx, int idx, hipStream_t st) {
  if (idx >= 0) (void)hipEventRecord(ctx->phase_events[idx].e1, st);
}
int phase_begin(hfmi_ctx* ctx, int phase) { return phase_begin_on(ctx, phase, ctx->stream); }
void phase_end(hfmi_ctx* ctx, int idx) { phase_end_on(ctx, idx, ctx->stream); }
extern "C" int hfmi_profile_phases(hfmi_ctx* ctx, double* ms_out) {
  if (!ctx || !ms_out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  for (int i = 0; i < HFMI_PHASE_COUNT; ++i) ms_out[i] = ctx->phase_ms[i];
  return HFMI_OK;
}
extern "C" int hfmi_profile_begin(hfmi_ctx* ctx) {
  if (!ctx) HFMI_FAIL(HFMI_ERR_INVALID, "null ctx");
  ctx->prof.clear();
  ctx->phase_events.clear();
  for (int i = 0; i < HFMI_PHASE_COUNT; ++i) ctx->phase_ms[i] = 0.0;
  ctx->profiling = true;
  return HFMI_OK;
}
extern "C" int hfmi_profile_end(hfmi_ctx* ctx, int max_groups, int* ngroups, int* kind, int64_t* shape, double* ms,
                                int64_t* launches, double* flops_per_launch, double* bytes_per_launch) {
  if (!ctx || !ngroups || !kind || !shape || !ms || !launches || !flops_per_launch || !bytes_per_launch)
    HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  ctx->profiling = false;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  int ng = 0;
  for (auto& r : ctx->prof) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.e0, r.e1) != hipSuccess) continue;
    int g = 0;
    for (; g < ng; ++g)
      if (kind[g] == r.kind && shape[3 * g] == r.m && shape[3 * g + 1] == r.k && shape[3 * g + 2] == r.N) break;
    if (g == ng) {
      if (ng >= max_groups) continue;
      kind[g] = r.kind;
      shape[3 * g] = r.m;
      shape[3 * g + 1] = r.k;
      shape[3 * g + 2] = r.N;
      ms[g] = 0.0;
      launches[g] = 0;
      flops_per_launch[g] = r.flops;
      bytes_per_launch[g] = r.bytes;
      ++ng;
    }
    ms[g] += t;
    launches[g] += 1;
  }
  ctx->prof.clear();
  for (auto& r : ctx->phase_events) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.e0, r.e1) == hipSuccess) ctx->phase_ms[r.phase] += t;
  }
  ctx->phase_events.clear();
  *ngroups = ng;
  return HFMI_OK;
}
