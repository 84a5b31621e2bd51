// Dynamic thresholding of the guided pred_xstart for DPM-Solver++ sampling (Saharia et al., 2022, "dynamic thresholding"; Lu et al., 2022):
// per sample b, with a_b = |x0c_b| flattened to n = 3 H W values and v_j its j-th smallest,
//   q_b = v_k + (v_{k+1} - v_k) frac        (torch.quantile's 'linear' rule; k, frac from the host: SpacedDiffusion.threshold_rank)
//   s_b = min(max(q_b, floor), cap)
//   x0t = clamp(x0c, -s_b, s_b) / s_b       (a true division), and x0t takes x0c's place in the update of dpm.hip.
// This file holds the selection; the thresholded update is the THR instantiation of dpmpp_update_kernel (dpm.hip), which reads the x0c buffer
// and thr3[b * 3 + 2] written here.
//      Selection: exact v_k and v_{k+1} by radix selection on the bit patterns with the sign cleared (non-negative IEEE floats order like
//      their unsigned bits), four 8-bit digits from the top.  A row is cut into slices of kSlice values, one workgroup of 256 threads per
//      (slice, row).  Launch p (p = 0 .. 3) counts digit p of the values whose higher digits equal the bins found so far in an integer LDS
//      histogram (1 KB) and writes its 256 counts to the caller's scratch with plain stores.  The NEXT launch sums the slices' counts in
//      slice order (every workgroup of the row does, redundantly: 256 threads, one bin each), scans them and finds the bin that holds rank
//      k; the workgroup of slice 0 records (bins so far, remaining rank) for the launch after that.  Launch 3 also takes, per slice, the
//      integer minimum of the patterns whose upper 24 bits exceed the ones found.  A fifth launch of one workgroup per row resolves the
//      last digit: v_k; v_{k+1} = v_k if more values equal v_k than the remaining rank needs (or k = n - 1), else the next non-empty bin
//      of the last histogram, else the minimum over the slices.  It writes thr3[b] = {v_k, v_{k+1}, s_b}.
//      There is NO cross-workgroup synchronisation inside a launch (no global atomics, tickets, flags or cooperative launches): whatever
//      one workgroup needs from another crosses a launch boundary.  All counts are integers and are summed in a fixed order, so the results
//      are the same bits on every run.  A row that holds NaN or infinity cannot fault (every pattern falls in some bin and the counts
//      still sum to n) and does not touch the other rows; its own result is unspecified.
//      On the sampler's data the first launch computes x0c from x, pred_xstart, g and scalars[7] (guided_x0 of guidance.h, exactly as
//      dpm.hip does) and WRITES it to a (B,3,H,W) buffer; the later launches and the update read that buffer, so the selected and the
//      clamped values are the same bits.  cgd_op_abs_quantile runs the same kernels on a plain [B][n] array.
//      With cap == floor every s_b is known (= cap): one launch writes x0c and thr3, and no selection launch runs.
// Scratch: (2 * B * S * 256 + 6 * B + B * S) uint32 with S = ceil(n / kSlice) (cgd_abs_quantile_scratch_bytes).  LDS: 1 KB histogram +
// 48 bytes.  All tensors fp32; any 4-byte-aligned pointers and any n (16-byte accesses when every pointer is 16-byte aligned and 4 | n).
#include "../../include/cgd_mi355x.h"
#include "common.h"
#include "elem_pack.h"
#include "guidance.h"

#include <algorithm>
#include <cmath>

namespace {

using namespace elem_pack;

constexpr int kSlice = 4096;  // values per workgroup: 16 KB, 16 per thread (four 16-byte units: the passes are bound by load latency, not bandwidth)
constexpr int kBins = 256;
constexpr unsigned kNone = 0xffffffffu;

struct SelArgs {
  // source: either a plain array (v) or the sampler's tensors, from which launch 0 computes x0c and stores it
  const float* v;        // launches 1..3 and the plain launch 0: [B][n]
  const float* x;        // guided launch 0
  const float* x0;
  const float* g;        // or null
  const float* scalars;  // or null
  float* x0c;            // guided launch 0 writes it
  unsigned* part;        // [2][B][S][256]: launch p writes half p & 1
  unsigned* state;       // [3][B][2]: (bins found so far, remaining rank) after digits 0, 1, 2
  unsigned* pmin;        // [B][S]
  float* thr;            // [B][3], written by the finishing launch (or by the guided launch when no selection runs)
  long n;
  unsigned k;
  int S;
  float frac, floor, cap;
};

__device__ __forceinline__ unsigned key_of(float f) { return __float_as_uint(f) & 0x7fffffffu; }

// One count per active lane into the LDS histogram.  The top digits of image data fall into a handful of bins, and 64 LDS atomics on one
// address serialise: the first lanes' bins are peeled off with one atomic per distinct bin (up to four rounds), the rest add singly.
// Must be called by every lane of the wavefront.
__device__ __forceinline__ void hist_add(unsigned* h, unsigned d, bool active) {
  const int lane = threadIdx.x & 63;
#pragma unroll 1
  for (int r = 0; r < 4; ++r) {
    const unsigned long long m = __ballot(active);
    if (!m) return;
    const int leader = __ffsll((long long)m) - 1;
    const unsigned d0 = (unsigned)__shfl((int)d, leader);
    const unsigned long long same = __ballot(active && d == d0);
    if (lane == leader) atomicAdd(&h[d0], (unsigned)__popcll(same));
    if (d == d0) active = false;
  }
  if (active) atomicAdd(&h[d], 1u);
}

// Sums the 256 counts of the S slices of one row in slice order (thread t: bin t), scans them and finds the bin that holds rank `rank`.
// Returns through LDS sel[4] = {bin, rank inside the bin, count of the bin, smallest non-empty bin above it or kNone}.  256 threads.
__device__ __forceinline__ void resolve(const unsigned* part_row, int S, unsigned rank, unsigned* wsum, unsigned* sel) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  unsigned c = 0;
  for (int s = 0; s < S; ++s) c += part_row[(long)s * kBins + t];
  unsigned inc = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned up = (unsigned)__shfl_up((int)inc, o);
    if (lane >= o) inc += up;
  }
  if (t == 0) {
    sel[0] = kBins - 1, sel[1] = 0, sel[2] = 0;
    sel[3] = kNone;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  unsigned before = 0;
  for (int j = 0; j < w; ++j) before += wsum[j];
  inc += before;
  const unsigned exc = inc - c;
  if (c != 0 && exc <= rank && rank < inc) sel[0] = t, sel[1] = rank - exc, sel[2] = c;  // exactly one thread: the counts sum past rank
  __syncthreads();
  if (c != 0 && (unsigned)t > sel[0]) atomicMin(&sel[3], (unsigned)t);
  __syncthreads();
}

// Launch p of the selection.  GUIDE (launch 0 on the sampler's data): the values are computed and stored first.  COUNT false: only that.
template <int V, bool GUIDE, bool COUNT>
__global__ __launch_bounds__(256) void thr_select_kernel(SelArgs a, StepCoef kc, int pass) {
  __shared__ unsigned hist[kBins];
  __shared__ unsigned wsum[4], sel[4], red[4];
  const int b = blockIdx.y, slice = blockIdx.x, B = gridDim.y, t = threadIdx.x;
  const long row = (long)b * a.n;
  unsigned prefix = 0;  // the bins found so far, as the upper 8 * pass bits of a pattern
  if (COUNT) {
    hist[t] = 0;
    if (pass > 0) {
      unsigned rank = a.k;
      if (pass > 1) {
        prefix = a.state[((long)(pass - 2) * B + b) * 2];
        rank = a.state[((long)(pass - 2) * B + b) * 2 + 1];
      }
      resolve(a.part + ((long)((pass - 1) & 1) * B + b) * a.S * kBins, a.S, rank, wsum, sel);
      prefix = (prefix << 8) | sel[0];
      if (slice == 0 && t == 0) {
        a.state[((long)(pass - 1) * B + b) * 2] = prefix;
        a.state[((long)(pass - 1) * B + b) * 2 + 1] = sel[1];
      }
    }
    __syncthreads();
  } else if (slice == 0 && t == 0) {
    a.thr[b * 3] = 0.f, a.thr[b * 3 + 1] = 0.f, a.thr[b * 3 + 2] = a.cap;
  }
  const int shift = 24 - 8 * pass;
  const float fct = (GUIDE && a.scalars) ? a.scalars[7] : 1.f;
  const long lo = (long)slice * kSlice, hi = std::min(a.n, lo + kSlice);
  unsigned above = kNone;
  for (long base = lo; base < hi; base += 256 * V) {  // wavefront-uniform trip count: hist_add is called by every lane
    const long e = base + (long)t * V;
    const bool in = e < hi;  // V = 4: n and kSlice are multiples of 4, a unit is whole or absent
    float val[V];
    if (in) {
      if (GUIDE) {
        float x[V], x0[V], g[V];
        load<V>(a.x + row + e, x);
        load<V>(a.x0 + row + e, x0);
        if (a.g) load<V>(a.g + row + e, g);
#pragma unroll
        for (int j = 0; j < V; ++j) val[j] = guided_x0(kc, x[j], x0[j], a.g ? g[j] * fct : 0.f);
        store<V>(a.x0c + row + e, val);
      } else {
        load<V>(a.v + row + e, val);
      }
    }
    if (COUNT) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const unsigned key = in ? key_of(val[j]) : 0u;
        const bool mine = in && (pass == 0 || (key >> (shift + 8)) == prefix);
        hist_add(hist, (key >> shift) & 255u, mine);
        if (pass == 3 && in && (key >> 8) > prefix) above = std::min(above, key);
      }
    }
  }
  if (!COUNT) return;
  __syncthreads();
  a.part[(((long)(pass & 1) * B + b) * a.S + slice) * kBins + t] = hist[t];
  if (pass == 3) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) above = std::min(above, (unsigned)__shfl_xor((int)above, o));
    if ((t & 63) == 0) red[t >> 6] = above;
    __syncthreads();
    if (t == 0) a.pmin[(long)b * a.S + slice] = std::min(std::min(red[0], red[1]), std::min(red[2], red[3]));
  }
}

// The finishing launch: one workgroup per row.
__global__ __launch_bounds__(256) void thr_finish_kernel(SelArgs a) {
  __shared__ unsigned wsum[4], sel[4], red[4];
  const int b = blockIdx.x, B = gridDim.x, t = threadIdx.x;
  const unsigned prefix = a.state[((long)2 * B + b) * 2], rank = a.state[((long)2 * B + b) * 2 + 1];
  resolve(a.part + ((long)B + b) * a.S * kBins, a.S, rank, wsum, sel);  // launch 3 wrote half 1
  unsigned above = kNone;
  for (int s = t; s < a.S; s += 256) above = std::min(above, a.pmin[(long)b * a.S + s]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) above = std::min(above, (unsigned)__shfl_xor((int)above, o));
  if ((t & 63) == 0) red[t >> 6] = above;
  __syncthreads();
  if (t != 0) return;
  above = std::min(std::min(red[0], red[1]), std::min(red[2], red[3]));
  const unsigned vk = (prefix << 8) | sel[0];
  unsigned vk1 = vk;
  if ((long)a.k + 1 < a.n && sel[1] + 1 >= sel[2]) {  // the value after the last one that equals v_k
    if (sel[3] != kNone)
      vk1 = (prefix << 8) | sel[3];
    else if (above != kNone)
      vk1 = above;
  }
  const float fk = __uint_as_float(vk), fk1 = __uint_as_float(vk1);
  const float q = fk + (fk1 - fk) * a.frac;
  a.thr[b * 3] = fk;
  a.thr[b * 3 + 1] = fk1;
  a.thr[b * 3 + 2] = fminf(fmaxf(q, a.floor), a.cap);
}

int slices_of(long n) { return (int)((n + kSlice - 1) / kSlice); }

// the checks the two selecting entry points share; B and n are known to be positive
int check_rank(cgd_ctx* ctx, const char* who, int B, long n, long k, float frac, float floor, float cap, const void* thr, const void* scratch) {
  const std::string w(who);
  if (B > 65535) CGD_FAIL(ctx, w + ": more than 65535 rows");
  if (n > INT32_MAX) CGD_FAIL(ctx, w + ": a row exceeds 2^31 - 1 values");
  if (k < 0 || k >= n) CGD_FAIL(ctx, w + ": the rank k lies outside [0, n)");
  if (!(frac >= 0.f && frac <= 1.f)) CGD_FAIL(ctx, w + ": frac lies outside [0, 1]");
  if (!(cap >= floor)) CGD_FAIL(ctx, w + ": cap < floor (or one of them is NaN)");
  if (!thr) CGD_FAIL(ctx, w + ": the [B][3] result buffer is required");
  if (cap > floor && !scratch) CGD_FAIL(ctx, w + ": the selection needs its scratch (cgd_abs_quantile_scratch_bytes)");
  return 0;
}

void carve(SelArgs& a, void* scratch, int B) {
  a.part = static_cast<unsigned*>(scratch);
  a.state = a.part + (long)2 * B * a.S * kBins;
  a.pmin = a.state + (long)6 * B;
}

template <int V>
void launch_rest(const SelArgs& a, int B, hipStream_t s) {
  const dim3 grid(a.S, B);
  const StepCoef none = {};
  for (int pass = 1; pass < 4; ++pass) CGD_LAUNCH((thr_select_kernel<V, false, true>), grid, dim3(256), 0, s, a, none, pass);
  CGD_LAUNCH(thr_finish_kernel, dim3(B), dim3(256), 0, s, a);
}

}  // namespace

int cgd_abs_quantile_slice(void) { return kSlice; }

int64_t cgd_abs_quantile_scratch_bytes(int B, int64_t n) {
  if (B <= 0 || n <= 0 || n > INT32_MAX) return -1;
  const int64_t S = slices_of(n);
  return 4 * ((int64_t)2 * B * S * kBins + (int64_t)6 * B + (int64_t)B * S);
}

int cgd_launch_abs_quantile(cgd_ctx* ctx, const float* v, int B, long n, long k, float frac, float floor, float cap, float* out3,
                            void* scratch, hipStream_t s) {
  if (B <= 0 || n <= 0) CGD_FAIL(ctx, "abs quantile: empty shape");
  if (!v) CGD_FAIL(ctx, "abs quantile: the values are required");
  CGD_TRY(check_rank(ctx, "abs quantile", B, n, k, frac, floor, cap, out3, scratch));
  if (!scratch) CGD_FAIL(ctx, "abs quantile: the selection needs its scratch (cgd_abs_quantile_scratch_bytes)");  // also with cap == floor
  SelArgs a = {};
  a.v = v, a.thr = out3, a.n = n, a.k = (unsigned)k, a.S = slices_of(n), a.frac = frac, a.floor = floor, a.cap = cap;
  carve(a, scratch, B);
  const StepCoef none = {};
  const dim3 grid(a.S, B);
  if (n % 4 == 0 && aligned16(v)) {
    CGD_LAUNCH((thr_select_kernel<4, false, true>), grid, dim3(256), 0, s, a, none, 0);
    launch_rest<4>(a, B, s);
  } else {
    CGD_LAUNCH((thr_select_kernel<1, false, true>), grid, dim3(256), 0, s, a, none, 0);
    launch_rest<1>(a, B, s);
  }
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

int cgd_launch_dpmpp_threshold(cgd_ctx* ctx, const float* x, const float* x0, const float* g, const float* scalars, float* x0c, int B, int H,
                               int W, const StepCoef& kc, long k, float frac, float floor, float cap, float* thr3, void* scratch,
                               hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0) CGD_FAIL(ctx, "dpmpp threshold: empty shape");
  if ((long)H * W > INT32_MAX / 3) CGD_FAIL(ctx, "dpmpp threshold: a sample exceeds 2^31 - 1 values");
  if (!x || !x0 || !x0c) CGD_FAIL(ctx, "dpmpp threshold: x, pred_xstart and x0c are required");
  if (x0c == x || x0c == x0 || (g && x0c == g)) CGD_FAIL(ctx, "dpmpp threshold: x0c may not alias an input");
  const long n = (long)3 * H * W;
  CGD_TRY(check_rank(ctx, "dpmpp threshold", B, n, k, frac, floor, cap, thr3, scratch));
  SelArgs a = {};
  a.v = x0c, a.x = x, a.x0 = x0, a.g = g, a.scalars = scalars, a.x0c = x0c, a.thr = thr3;
  a.n = n, a.k = (unsigned)k, a.S = slices_of(n), a.frac = frac, a.floor = floor, a.cap = cap;
  const bool select = cap > floor, vec = n % 4 == 0 && aligned16(x) && aligned16(x0) && aligned16(g) && aligned16(x0c);
  if (select) carve(a, scratch, B);
  const dim3 grid(a.S, B);
  if (!select) {  // s_b = cap for every sample: x0c and thr3 are written, nothing is selected
    if (vec)
      CGD_LAUNCH((thr_select_kernel<4, true, false>), grid, dim3(256), 0, s, a, kc, 0);
    else
      CGD_LAUNCH((thr_select_kernel<1, true, false>), grid, dim3(256), 0, s, a, kc, 0);
  } else if (vec) {
    CGD_LAUNCH((thr_select_kernel<4, true, true>), grid, dim3(256), 0, s, a, kc, 0);
    launch_rest<4>(a, B, s);
  } else {
    CGD_LAUNCH((thr_select_kernel<1, true, true>), grid, dim3(256), 0, s, a, kc, 0);
    launch_rest<1>(a, B, s);
  }
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
