// Whittle-Matern priors on a box by DCT and FFT (hfmi_box_*, hfmi_op_box): the operator (delta - gamma div Theta grad)^(-alpha) on a
// regular grid with Neumann or periodic sides and axis-aligned Theta is diagonalised by cosine and Fourier transforms, so the covariance
// C, the precision R = C^-1 and the factors C^(1/2), C^(-1/2) are each one transform - multiply - inverse transform:
//   W^a T_s W^b,   T_s x = restrict( IFFT_unnormalised( (lambda^s / prod P_c) . FFT( extend(x) ) ) ),
// W the diagonal of quadrature weights, extend the even mirror of every Neumann axis, restrict the first n_c positions.  Nothing is
// grown, clipped, iterated or approximated, and the work buffer of a pair of columns has N entries.  What is planned where, the pass list
// and what a pass does at the ends of a line is in hfmi_boxcov_plan.h; this unit holds the kernels, the box's state and the launcher.
//
// k_boxcov_pass: `lpw` lines along one axis, one workgroup, the lines in LDS; the radix-4 and radix-2 stages and the quarter twiddle
// table are the ones k_fftcov_pass (hfmi_fftcov.hip) runs, and live in hfmi_fft_lds.h.  What differs from that kernel is the ends: a
// Neumann axis is mirrored into LDS on its time-side load, which makes the complex FFT a DCT-I of the real and of the imaginary part,
// and only its n modes are kept in the buffer; the line map divides, because strides are products of n_b and no powers of two; the
// scatter from the input block and the gather into the output block are fused into the first load and the last store, with W^b and W^a
// multiplied in there (the weight of a node is a product of per-axis end factors, counted from its indices: no scaling launch).
// Two real columns ride one transform, z = x_j + i x_{j+1}; the table is real, so the result is y_j + i y_{j+1}.  Every entry of Y is
// written by exactly one thread and there are no atomics: two applies are bit-identical, and the pairs per chunk ("fftcov_pairs")
// change nothing but the number of launches.
//
// k_boxcov_pass_mr: the same pass for a MIXED-RADIX line, P = 3^a 5^b Q entries with the power-of-two tail Q >= 4 (the rule of an axis,
// the order of the stages and the position map: hfmi_boxcov_plan.h).  Forward it runs one radix-3 or radix-5 stage per odd factor, then
// the radix-4 / radix-2 stages on every block of Q entries; the inverse is the transposed stages in reverse order (hfmi_fft_lds.h: the
// odd stage, and the power-of-two stages BLOCKED).  The ends are k_boxcov_pass's with the bit reversal replaced by the position map, read
// from a table built on the host (mode[p] and pos[m]); twiddles come from a quarter table of the line's own length.  Both kernels are one
// body (boxcov_pass_body<MR>): what MR changes is how an entry splits into (line, position), the position map, the twiddle staging and
// the odd stages.  A pass along an axis whose line is a power of two launches k_boxcov_pass with the twiddle table and shape it always
// had, also in a grid whose other axes are mixed-radix: its results are bit for bit what they were.
//
// LDS: lpw * (L + pad) entries of 16 bytes and the twiddles, dynamic; 256 line bases and 256 end counts, static (3 KiB).  The plan keeps
// static + dynamic within the 160 KiB of a workgroup (the longest line, 4096 entries, is 64 KiB).  The bank layout (the pad of
// fftcov_pass_shape; the mirrored and bit-reversed LDS stores of this kernel; the odd stages of k_boxcov_pass_mr, whose strides B / r
// are no powers of two, and its permuted stores) and the lines per workgroup have NOT been measured; docs/measurements.md has the
// apply times of both kernels as they stand.
//
// k_boxcov_table fills the table of one operator, lambda^s / prod P_c, one double per buffer entry in the buffer's order: natural k on
// a Neumann axis, the mode of the storage position on a periodic one (its bit reversal, or mode[p] of a mixed-radix line).  Built once
// per operator.
#include <math.h>

#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include "hfmi_boxcov_plan.h"
#include "hfmi_fft_lds.h"
#include "hfmi_internal.h"

struct boxcov_state {
  int d = 0;
  int64_t n[3] = {1, 1, 1};
  double h[3] = {1.0, 1.0, 1.0};
  int boundary[3] = {BOXCOV_NEUMANN, BOXCOV_NEUMANN, BOXCOV_NEUMANN};
  double theta[3] = {1.0, 1.0, 1.0};
  double gamma = 1.0, delta = 1.0, alpha = 2.0;
  int symbol = HFMI_BOX_SYMBOL_FD;
  int64_t N = 0;
  dev_buf<double2> tw;     // the power-of-two lines' table: exp(-2 pi i k / Pmax), k < max(Pmax / 4, 1)
  // mixed-radix axes: slot of the axis (-1: a power-of-two line), axes of one length share a slot; per slot the quarter table
  // exp(-2 pi i k / P), k < P / 4, and the position map, mode[p] then pos[m] (boxcov_mr_modes)
  int mr_slot[3] = {-1, -1, -1};
  dev_buf<double2> mr_tw[3];
  dev_buf<int> mr_map[3];
  dev_buf<double2> work;   // arrays of N entries, one per pair of a chunk (fft_fit_work)
  boxcov_plan plan;
};

struct hfmi_box {
  hfmi_ctx* ctx = nullptr;
  std::shared_ptr<boxcov_state> st;     // shared with the operators made from this box (hfmi_op_box)
};

struct boxcov_pass_args {
  double2* buf;
  int64_t pair_stride;     // entries between the arrays of consecutive pairs: N
  const double2* tw;
  int tw_step;             // Pmax / L
  const double* table;
  int flags, L, logL, n, mirror, lpw, loglpw, ls;
  int64_t stride, span, nlines;
  int n1, n2;              // scatter / gather (a pass along axis 0): line l is (i1, i2) = (l mod n1, l div n1)
  int end0, end1, end2;    // 1: the axis is Neumann with more than one node, its two end nodes carry half a weight
  double wl[4], ws[4];     // (w_interior / 2^c)^a and ^b for a node that is an end node on c axes
  const double* W;
  int64_t ldw;
  double* Y;
  int64_t ldy;
  int ncols, col0, accumulate;
};

// mixed-radix lines: L = 3^n3 5^n5 2^logQ (hfmi_boxcov_plan.h)
struct boxcov_mr_args {
  boxcov_pass_args a;      // tw: the quarter table of this length, exp(-2 pi i k / L), k < L / 4; tw_step and logL are not read
  const int* mode;         // mode[p], p < L: the mode at position p after the forward stages; then pos[m], m < L: its inverse
  int n3, n5, logQ;
};

// reversal of the low logL bits; logL = 0: the single position 0
__device__ __forceinline__ int bc_brev(int p, int logL) { return logL ? (int)(__brev((unsigned)p) >> (32 - logL)) : 0; }

// The pass of both kernels.  MR: a mixed-radix line L = 3^n3 5^n5 2^logQ: the line of an entry is found by dividing (L is no power of
// two), the position map and its inverse come from `mode` in place of the bit reversal, the twiddles are the line's own quarter table,
// and the odd stages stand around the power-of-two stages, which run on the L / Q blocks of Q entries (hfmi_fft_lds.h: BLOCKED).
// Otherwise logQ = logL, `mode` is not read and the pass compiles to the power-of-two code it always was.
template <bool MR>
__device__ __forceinline__ void boxcov_pass_body(const boxcov_pass_args& A, const int* mode, int n3, int n5, int logQ) {
  extern __shared__ double2 bc_lds[];
  __shared__ int64_t lbase[FFTCOV_MAX_LINES];    // first entry of the line in the pair's array (= its first node on axis 0), -1: no such line
  __shared__ int lends[FFTCOV_MAX_LINES];        // axis-0 lines: on how many of the axes 1, 2 the line's nodes are end nodes
  const int tid = threadIdx.x, nt = blockDim.x;
  const int L = A.L, lpw = A.lpw, ls = A.ls, n = A.n;
  // the mode at LDS position p after the forward stages, and the LDS position of mode m
  const auto mode_at = [&](int p) { return MR ? mode[p] : bc_brev(p, logQ); };
  const auto pos_of = [&](int m) { return MR ? mode[L + m] : bc_brev(m, logQ); };
  double2* x = bc_lds;
  double2* ltw = bc_lds + lpw * ls;
  const int qm = L / 4 > 1 ? L / 4 : 1;
  const int64_t line0 = (int64_t)blockIdx.x * lpw;
  const int pair = blockIdx.y;
  double2* buf = A.buf + (int64_t)pair * A.pair_stride;
  const bool ends = (A.flags & (FFTCOV_SCATTER | FFTCOV_GATHER)) != 0;
  for (int j = tid; j < lpw; j += nt) {
    const int64_t line = line0 + j;
    int64_t b = -1;
    int c = 0;
    if (line < A.nlines) {
      const int64_t o = line / A.stride, inner = line - o * A.stride;
      b = inner + o * A.span;
      if (ends) {
        const int64_t i2 = line / A.n1, i1 = line - i2 * A.n1;
        c = (A.end1 && (i1 == 0 || i1 == A.n1 - 1)) + (A.end2 && (i2 == 0 || i2 == A.n2 - 1));
      }
    }
    lbase[j] = b;
    lends[j] = c;
  }
  for (int i = tid; i < qm; i += nt) ltw[i] = A.tw[MR ? (int64_t)i : (int64_t)i * A.tw_step];
  __syncthreads();

  // entry e of the workgroup's lines -> (line j, position p): along the line on the contiguous axis, across adjacent lines on a strided one
  const int total = MR ? lpw * L : lpw << logQ;
  const bool strided = A.stride > 1;
  const auto entry = [&](int e, int& j, int& p) {
    if (strided) j = e & (lpw - 1), p = e >> A.loglpw;
    else fft_split<MR>(e, L, logQ, j, p);
  };
  const int c0 = A.col0 + 2 * pair;
  const bool has1 = c0 + 1 < A.ncols;
  const bool fwd = (A.flags & FFTCOV_FWD) != 0, inv = (A.flags & FFTCOV_INV) != 0;

  // load: the first n positions of the buffer's line (time side: nodes; frequency side: modes), each to the LDS positions it stands for
  for (int e = tid; e < total; e += nt) {
    int j, p;
    entry(e, j, p);
    if (p >= n) continue;
    double2 v = double2{0.0, 0.0};
    const int64_t b = lbase[j];
    if (b >= 0) {
      if (A.flags & FFTCOV_SCATTER) {
        const int64_t node = b + p;
        const double w = A.ws[lends[j] + (A.end0 && (p == 0 || p == n - 1))];
        v.x = A.W[(int64_t)c0 * A.ldw + node] * w;
        if (has1) v.y = A.W[(int64_t)(c0 + 1) * A.ldw + node] * w;
      } else {
        v = buf[b + (int64_t)p * A.stride];
      }
    }
    double2* xl = x + j * ls;
    if (!A.mirror) {
      xl[p] = v;
    } else if (fwd) {
      xl[p] = v;
      if (p >= 1 && p <= n - 2) xl[L - p] = v;
    } else {
      xl[pos_of(p)] = v;
      if (p >= 1 && p <= n - 2) xl[pos_of(L - p)] = v;
    }
  }
  __syncthreads();

  if (fwd) {
    if constexpr (MR) {
      int B = L;
      for (int s = 0; s < n3; ++s, B /= 3) fft_odd_stage<3, false>(x, ltw, L, B, lpw, ls, tid, nt);
      for (int s = 0; s < n5; ++s, B /= 5) fft_odd_stage<5, false>(x, ltw, L, B, lpw, ls, tid, nt);
    }
    fft_pow2_forward<MR>(x, ltw, qm, L, logQ, lpw, ls, tid, nt);
  }

  if (A.flags & FFTCOV_MUL) {
    // LDS position p holds the mode mode_at(p) of the full line; a Neumann axis keeps the modes 0 .. n - 1 = P / 2 and the rest mirror them
    for (int e = tid; e < total; e += nt) {
      int j, p;
      entry(e, j, p);
      const int64_t b = lbase[j];
      if (b >= 0) {
        int k = p;
        if (A.mirror) {
          const int m = mode_at(p);
          k = m < L - m ? m : L - m;
        }
        const double lam = A.table[b + (int64_t)k * A.stride];
        double2 v = x[j * ls + p];
        v.x *= lam;
        v.y *= lam;
        x[j * ls + p] = v;
      }
    }
    __syncthreads();
  }

  if (inv) {
    fft_pow2_inverse<MR>(x, ltw, qm, L, logQ, lpw, ls, tid, nt);
    if constexpr (MR) {
      int B = 1 << logQ;     // the odd stages in reverse order: the radix-5 blocks from the smallest, then the radix-3 ones
      for (int s = 0; s < n5; ++s) fft_odd_stage<5, true>(x, ltw, L, B *= 5, lpw, ls, tid, nt);
      for (int s = 0; s < n3; ++s) fft_odd_stage<3, true>(x, ltw, L, B *= 3, lpw, ls, tid, nt);
    }
  }

  // store: the first n positions of the buffer's line; after the inverse stages they are the nodes, after the forward stages the modes
  for (int e = tid; e < total; e += nt) {
    int j, p;
    entry(e, j, p);
    const int64_t b = lbase[j];
    if (b < 0 || p >= n) continue;
    const double2 v = x[j * ls + ((A.mirror && !inv) ? pos_of(p) : p)];
    if (A.flags & FFTCOV_GATHER) {
      const int64_t node = b + p;
      const double w = A.wl[lends[j] + (A.end0 && (p == 0 || p == n - 1))];
      // the product is rounded before it is added (no fused multiply-add): an accumulating apply adds exactly what an overwriting one stores
      const double r0 = __dmul_rn(w, v.x), r1 = __dmul_rn(w, v.y);
      double* y0 = A.Y + (int64_t)c0 * A.ldy + node;
      *y0 = A.accumulate ? *y0 + r0 : r0;
      if (has1) {
        double* y1 = y0 + A.ldy;
        *y1 = A.accumulate ? *y1 + r1 : r1;
      }
    } else {
      buf[b + (int64_t)p * A.stride] = v;
    }
  }
}

__global__ __launch_bounds__(FFTCOV_MAX_THREADS) void k_boxcov_pass(boxcov_pass_args A) { boxcov_pass_body<false>(A, nullptr, 0, 0, A.logL); }
__global__ __launch_bounds__(FFTCOV_MAX_THREADS) void k_boxcov_pass_mr(boxcov_mr_args M) {
  boxcov_pass_body<true>(M.a, M.mode, M.n3, M.n5, M.logQ);
}

struct boxcov_table_args {
  int n[3], logP[3], periodic[3], continuous;
  const int* mode[3];      // a periodic mixed-radix axis: mode[p] of its storage position; null: the bit reversal
  double h[3], theta[3];
  double gamma, delta, expo, scale;     // table = (delta + gamma sum theta mu)^expo * scale, expo = -alpha s, scale = 1 / prod P_c
};
// mu_c of mode k: "fd" (2 - 2 cos t) / h^2, evaluated as (2 sin(t / 2) / h)^2, which is the same number without the cancellation at
// small t; "continuous" (t / h)^2.  t = pi k / (n - 1) on a Neumann axis, 2 pi k~ / n with the signed k~ on a periodic one.
__device__ __forceinline__ double bc_mu(const boxcov_table_args& T, int c, int e) {
  double half_over_pi;      // t / (2 pi)
  if (T.periodic[c]) {
    const int k = T.mode[c] ? T.mode[c][e] : T.logP[c] ? (int)(__brev((unsigned)e) >> (32 - T.logP[c])) : 0;
    const int ks = 2 * k <= T.n[c] ? k : k - T.n[c];
    half_over_pi = (double)ks / (double)T.n[c];
  } else {
    half_over_pi = T.n[c] > 1 ? (double)e / (double)(2 * (T.n[c] - 1)) : 0.0;
  }
  const double r = T.continuous ? 2.0 * 3.141592653589793238 * half_over_pi : 2.0 * sinpi(half_over_pi);
  const double q = r / T.h[c];
  return q * q;
}
__global__ __launch_bounds__(256) void k_boxcov_table(boxcov_table_args T, double* table, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int e0 = (int)(e % T.n[0]);
    const int64_t r = e / T.n[0];
    const int e1 = (int)(r % T.n[1]), e2 = (int)(r / T.n[1]);
    double sum = T.theta[0] * bc_mu(T, 0, e0);
    sum = fma(T.theta[1], bc_mu(T, 1, e1), sum);
    sum = fma(T.theta[2], bc_mu(T, 2, e2), sum);
    table[e] = pow(fma(T.gamma, sum, T.delta), T.expo) * T.scale;
  }
}

// ------------------------------------------------------------------ host
static bool bc_positive(double v) { return v > 0.0 && isfinite(v); }

static int boxcov_check_grid(const char* who, int d, const int64_t* n, const int* boundary) {
  if (!n || !boundary) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (d < 1 || d > 3) HFMI_FAIL(HFMI_ERR_INVALID, "%s: d = %d is not 1, 2 or 3", who, d);
  for (int c = 0; c < d; ++c) {
    if (boundary[c] != BOXCOV_NEUMANN && boundary[c] != BOXCOV_PERIODIC)
      HFMI_FAIL(HFMI_ERR_INVALID, "%s: boundary[%d] = %d is not 0 (Neumann) or 1 (periodic)", who, c, boundary[c]);
    if (!boxcov_axis_ok(n[c], boundary[c]))
      HFMI_FAIL(HFMI_ERR_INVALID,
                "%s: n[%d] = %lld: the line of an axis, 2 (n - 1) entries on a Neumann axis of n > 1 nodes and n on a periodic one, is a power of "
                "two or a multiple of 4 with no prime factor but 2, 3 and 5; a Neumann axis has at most %d nodes, a periodic one %d",
                who, c, (long long)n[c], BOXCOV_MAX_NEUMANN, BOXCOV_MAX_PERIODIC);
  }
  return HFMI_OK;
}

extern "C" int hfmi_boxcov_plan_predict(int d, const int64_t* n, const int* boundary, int nvec, int64_t budget_bytes, int64_t* words) {
  if (!words) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  HFMI_TRY(boxcov_check_grid("boxcov_plan_predict", d, n, boundary));
  if (nvec < 0) HFMI_FAIL(HFMI_ERR_INVALID, "boxcov_plan_predict: negative number of vectors");
  boxcov_plan p = boxcov_plan_passes(d, n, boundary);
  fftcov_plan_chunks(p.chunks, nvec, budget_bytes, fftcov_pairs_knob());
  boxcov_plan_words(p, words);
  return HFMI_OK;
}
static_assert(BOXCOV_PLAN_WORDS == HFMI_BOXCOV_PLAN_WORDS, "include/hfmi.h sizes the array of hfmi_boxcov_plan_predict");
static_assert(BOXCOV_NEUMANN == HFMI_BOX_NEUMANN && BOXCOV_PERIODIC == HFMI_BOX_PERIODIC, "the plan header restates include/hfmi.h");

static int box_create(hfmi_ctx* ctx, int d, const int64_t* n, const double* h, const int* boundary, double gamma, double delta, double alpha,
                      const double* theta_or_null, int symbol, hfmi_box** out) {
  if (!ctx || !h || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  HFMI_TRY(boxcov_check_grid("box_create", d, n, boundary));
  for (int c = 0; c < d; ++c) {
    if (!bc_positive(h[c])) HFMI_FAIL(HFMI_ERR_INVALID, "box_create: spacing h[%d] must be positive and finite", c);
    if (theta_or_null && !bc_positive(theta_or_null[c])) HFMI_FAIL(HFMI_ERR_INVALID, "box_create: theta[%d] must be positive and finite", c);
  }
  if (!bc_positive(gamma) || !bc_positive(delta) || !bc_positive(alpha))
    HFMI_FAIL(HFMI_ERR_INVALID, "box_create: gamma, delta and alpha must be positive and finite");
  if (symbol != HFMI_BOX_SYMBOL_FD && symbol != HFMI_BOX_SYMBOL_CONTINUOUS)
    HFMI_FAIL(HFMI_ERR_INVALID, "box_create: symbol = %d is not 0 (fd) or 1 (continuous)", symbol);
  // host allocations here (the box, its shared state with the control block, the twiddle vector) may throw: hfmi_box_create catches
  std::unique_ptr<hfmi_box> box(new hfmi_box());
  box->ctx = ctx;
  box->st = std::make_shared<boxcov_state>();
  boxcov_state* st = box->st.get();
  st->d = d;
  for (int c = 0; c < d; ++c) st->n[c] = n[c], st->h[c] = h[c], st->boundary[c] = boundary[c], st->theta[c] = theta_or_null ? theta_or_null[c] : 1.0;
  st->gamma = gamma, st->delta = delta, st->alpha = alpha, st->symbol = symbol;
  st->plan = boxcov_plan_passes(d, n, boundary);
  st->N = st->plan.N;
  const boxcov_plan& p = st->plan;
  for (int i = 0; i < p.npasses; ++i)
    if (!boxcov_pass_launchable(p.pass[i]))
      HFMI_FAIL(HFMI_ERR_INVALID, "box_create: pass %d (%d lines x %d entries, %d bytes of LDS, grid %lld) cannot be launched", i, p.pass[i].lpw,
                p.pass[i].L, p.pass[i].lds, (long long)p.pass[i].grid_x);
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipFuncSetAttribute((const void*)k_boxcov_pass, hipFuncAttributeMaxDynamicSharedMemorySize, FFTCOV_LDS_BYTES - BOXCOV_STATIC_LDS));
  HIP_TRY(hipFuncSetAttribute((const void*)k_boxcov_pass_mr, hipFuncAttributeMaxDynamicSharedMemorySize, FFTCOV_LDS_BYTES - BOXCOV_STATIC_LDS));
  const hipError_t e = (hipError_t)st->work.alloc((size_t)p.chunks.pair_bytes / sizeof(double2));
  if (e != hipSuccess)
    HFMI_FAIL(HFMI_ERR_HIP, "box_create: the grid %lld x %lld x %lld needs %lld bytes of work buffer per pair of vectors: %s", (long long)p.n[0],
              (long long)p.n[1], (long long)p.n[2], (long long)p.chunks.pair_bytes, hipGetErrorString(e));
  HFMI_TRY(fft_twiddles_upload(st->tw, p.Pmax, p.twiddles));
  // every distinct mixed-radix length: its own quarter table and its position map
  int slots = 0;
  for (int c = 0; c < d; ++c) {
    int n3, n5, logQ;
    const int P = p.P[c];
    if (!boxcov_mr_factor(P, &n3, &n5, &logQ)) continue;
    for (int b = 0; b < c; ++b)
      if (p.P[b] == P) st->mr_slot[c] = st->mr_slot[b];
    if (st->mr_slot[c] >= 0) continue;
    const int slot = st->mr_slot[c] = slots++;
    std::vector<int> map(2 * (size_t)P);
    boxcov_mr_modes(P, map.data(), map.data() + P);
    HFMI_TRY(fft_twiddles_upload(st->mr_tw[slot], P, P / 4));
    OWN_TRY(st->mr_map[slot].alloc(map.size()));
    HIP_TRY(hipMemcpy(st->mr_map[slot], map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  *out = box.release();
  return HFMI_OK;
}
// no exception crosses the C ABI: a failed host allocation is an error code, and what was made so far is freed by its owners
extern "C" int hfmi_box_create(hfmi_ctx* ctx, int d, const int64_t* n, const double* h, const int* boundary, double gamma, double delta,
                               double alpha, const double* theta_or_null, int symbol, hfmi_box** out) {
  try {
    return box_create(ctx, d, n, h, boundary, gamma, delta, alpha, theta_or_null, symbol, out);
  } catch (const std::bad_alloc&) {
    HFMI_FAIL(HFMI_ERR_INVALID, "box_create: out of host memory");
  }
}

extern "C" int hfmi_box_destroy(hfmi_box* box) {
  if (!box) return HFMI_OK;
  (void)hipStreamSynchronize(box->ctx->stream);     // applies queued so far use the buffers
  delete box;
  return HFMI_OK;
}

// mu_c of the natural mode k on the host: the formulas of bc_mu
static double boxcov_mu_host(const boxcov_state* st, int c, int64_t k) {
  const long double pi = acosl(-1.0L);
  const int64_t nc = st->n[c];
  long double t;
  if (st->boundary[c] == BOXCOV_PERIODIC) t = 2.0L * pi * (long double)(2 * k <= nc ? k : k - nc) / (long double)nc;
  else t = nc > 1 ? pi * (long double)k / (long double)(nc - 1) : 0.0L;
  const long double r = st->symbol == HFMI_BOX_SYMBOL_CONTINUOUS ? t : 2.0L * sinl(0.5L * t);
  const long double q = r / (long double)st->h[c];
  return (double)(q * q);
}

extern "C" int hfmi_box_spectrum(const hfmi_box* box, double* lambda) {
  if (!box || !lambda) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  const boxcov_state* st = box->st.get();
  for (int64_t k2 = 0; k2 < st->n[2]; ++k2)
    for (int64_t k1 = 0; k1 < st->n[1]; ++k1)
      for (int64_t k0 = 0; k0 < st->n[0]; ++k0) {
        const double sum = st->theta[0] * boxcov_mu_host(st, 0, k0) + st->theta[1] * boxcov_mu_host(st, 1, k1) + st->theta[2] * boxcov_mu_host(st, 2, k2);
        lambda[k0 + st->n[0] * (k1 + st->n[1] * k2)] = pow(st->delta + st->gamma * sum, -st->alpha);
      }
  return HFMI_OK;
}

extern "C" int hfmi_op_box(hfmi_box* box, double s, double a, double b, hfmi_op** out) {
  if (!box || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (!isfinite(s) || !isfinite(a) || !isfinite(b)) HFMI_FAIL(HFMI_ERR_INVALID, "op_box: the powers s, a and b must be finite");
  hfmi_ctx* ctx = box->ctx;
  boxcov_state* st = box->st.get();
  HIP_TRY(hipSetDevice(ctx->device));
  std::unique_ptr<hfmi_op> op(new (std::nothrow) hfmi_op());
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->ctx = ctx;
  op->kind = OP_BOX;
  op->box = box->st;
  op->box_a = a, op->box_b = b;
  const hipError_t e = (hipError_t)op->box_table.alloc((size_t)st->N);
  if (e != hipSuccess) HFMI_FAIL(HFMI_ERR_HIP, "op_box: the table of %lld modes needs %lld bytes: %s", (long long)st->N, (long long)(st->N * 8), hipGetErrorString(e));
  boxcov_table_args T;
  double Ptot = 1.0;
  for (int c = 0; c < 3; ++c) {
    T.n[c] = (int)st->n[c], T.logP[c] = fftcov_log2(st->plan.P[c]);
    T.periodic[c] = st->boundary[c] == BOXCOV_PERIODIC;
    T.mode[c] = T.periodic[c] && st->mr_slot[c] >= 0 ? st->mr_map[st->mr_slot[c]].get() : nullptr;
    T.h[c] = st->h[c];
    T.theta[c] = c < st->d ? st->theta[c] : 0.0;
    Ptot *= (double)st->plan.P[c];
  }
  T.continuous = st->symbol == HFMI_BOX_SYMBOL_CONTINUOUS;
  T.gamma = st->gamma, T.delta = st->delta, T.expo = -st->alpha * s, T.scale = 1.0 / Ptot;
  const int64_t blocks = std::min<int64_t>((st->N + 255) / 256, (int64_t)ctx->num_cus * 8);
  hipLaunchKernelGGL(k_boxcov_table, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, T, op->box_table.get(), st->N);
  const hipError_t launched = hipGetLastError();
  const hipError_t done = hipStreamSynchronize(ctx->stream);   // whatever happened: the table must not go while a kernel may write it
  HIP_TRY(launched);
  HIP_TRY(done);
  *out = op.release();
  return HFMI_OK;
}

int64_t boxcov_points(const boxcov_state* st) { return st->N; }

int boxcov_apply(hfmi_ctx* ctx, boxcov_state* st, const double* table, double a, double b, const double* W, int64_t ldw, double* Y,
                 int64_t ldy, int nvec, int accumulate) {
  if (nvec < 1) return HFMI_OK;
  boxcov_plan p = st->plan;
  HFMI_TRY(fft_fit_work(ctx, st->work, p.chunks, st->N, nvec));
  // the weight of a node: prod_c w_c, w_c = h_c on a periodic axis, 1 on a Neumann axis of one node, h_c (halved at both ends) otherwise
  double w0 = 1.0;
  int end[3];
  for (int c = 0; c < 3; ++c) {
    end[c] = st->boundary[c] == BOXCOV_NEUMANN && st->n[c] > 1;
    if (c < st->d && (st->boundary[c] == BOXCOV_PERIODIC || st->n[c] > 1)) w0 *= st->h[c];
  }
  boxcov_pass_args A;
  A.pair_stride = st->N;
  A.tw = st->tw;
  A.table = table;
  A.n1 = (int)st->n[1], A.n2 = (int)st->n[2];
  A.end0 = end[0], A.end1 = end[1], A.end2 = end[2];
  for (int c = 0; c < 4; ++c) {
    const double w = ldexp(w0, -c);
    A.wl[c] = a == 0.0 ? 1.0 : pow(w, a);
    A.ws[c] = b == 0.0 ? 1.0 : pow(w, b);
  }
  A.W = W, A.ldw = ldw, A.Y = Y, A.ldy = ldy, A.ncols = nvec, A.accumulate = accumulate;
  for (int c = 0; c < p.chunks.nchunks; ++c) {
    const int pair0 = c * p.chunks.chunk_pairs, pairs = std::min(p.chunks.chunk_pairs, p.chunks.pairs - pair0);
    if (pairs > 65535) HFMI_FAIL(HFMI_ERR_INVALID, "op_box: %d pairs in one launch", pairs);
    A.buf = st->work;
    A.col0 = 2 * pair0;
    for (int i = 0; i < p.npasses; ++i) {
      const boxcov_pass& q = p.pass[i];
      if (!boxcov_pass_launchable(q))
        HFMI_FAIL(HFMI_ERR_INVALID, "op_box: pass %d (%d lines x %d entries, %d bytes of LDS) cannot be launched", i, q.lpw, q.L, q.lds);
      A.tw_step = p.Pmax / q.L;
      A.flags = q.flags, A.L = q.L, A.logL = q.logL, A.n = q.n, A.mirror = q.mirror, A.lpw = q.lpw, A.loglpw = q.loglpw, A.ls = q.ls;
      A.stride = q.stride, A.span = q.span, A.nlines = q.nlines;
      if (q.n3 + q.n5 > 0) {
        const int slot = st->mr_slot[q.axis];
        boxcov_mr_args M;
        M.a = A;
        M.a.tw = st->mr_tw[slot];
        M.mode = st->mr_map[slot];
        M.n3 = q.n3, M.n5 = q.n5, M.logQ = q.logQ;
        hipLaunchKernelGGL(k_boxcov_pass_mr, dim3((unsigned)q.grid_x, (unsigned)pairs), dim3(q.threads), (size_t)q.lds, ctx->stream, M);
      } else {
        hipLaunchKernelGGL(k_boxcov_pass, dim3((unsigned)q.grid_x, (unsigned)pairs), dim3(q.threads), (size_t)q.lds, ctx->stream, A);
      }
      HIP_TRY(hipGetLastError());
    }
  }
  return HFMI_OK;
}
