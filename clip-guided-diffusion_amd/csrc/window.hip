// Windowed sampling (MultiDiffusion, Bar-Tal et al., 2023): the frame is cut into overlapping S x S windows, the model runs on the windows as
// one batch, and the window outputs are averaged back into the frame.  Two kernels that form an adjoint pair:
//   gather  win[b,k,c,u,v]  = ay[ky][u] ax[kx][v] full[b,c,(oy[ky]+u) mod H,(ox[kx]+v) mod W]          k = ky * nx + kx
//   merge   full[b,c,y,x] (+)= sum_ky sum_kx ay[ky][u] ax[kx][v] win[b,k,c,u,v]   over the windows that cover (y,x): u = (y-oy[ky]) mod H < S, v likewise
// full: NCHW fp32 (B,C,H,W); win: (B*nW,C,S,S), row b*nW + k; oy / ox: window origins per axis (host arrays, at most 16 each, they travel in the
// kernel arguments); ay [ny][S], ax [nx][S]: device tables of per-axis weights, null = ones; wrap bit 0 / 1: windows run over the right / bottom
// edge and continue at index 0.  The merge is a gather too: one thread owns its output elements and walks the covering windows, ky ascending
// outside, kx ascending inside; no atomics, the same bits on every run.
// S, H, W and every origin are multiples of 8, so a unit of four consecutive x shares one covering set and never straddles a window edge or the
// wrap: it moves as one 16-byte access (V = 4; V = 1 when a pointer is only 4-byte aligned).  A workgroup takes `rpw` rows of one plane at a time
// (plane and row are decoded per workgroup, from uniform values), a thread one unit of one of those rows.
#include <string>
#include <vector>

#include "../../include/cgd_mi355x.h"
#include "common.h"
#include "elem_pack.h"
#include "kernels.h"

namespace {

using namespace elem_pack;

constexpr int kMaxWin = 16;  // windows per axis

struct WindowArgs {
  const float* ay;  // [ny][S] or null
  const float* ax;  // [nx][S] or null
  int oy[kMaxWin], ox[kMaxWin];
  int ny, nx;
  int planes;  // gather: B * nW * C window planes; merge: B * C frame planes
  int C, H, W, S, wrap;
  int upr, rpw, chunks;  // units per row of the walked tensor, rows per workgroup pass, passes per plane
};

// thread -> (row within the pass, first unit of the row); a row longer than 256 units is walked by the whole workgroup
__device__ __forceinline__ void thread_slot(const WindowArgs& a, int& r_local, int& u0) {
  r_local = threadIdx.x / a.upr;
  u0 = threadIdx.x - r_local * a.upr;
}

template <int V>
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ full, float* __restrict__ win, WindowArgs a) {
  int r_local, u0;
  thread_slot(a, r_local, u0);
  const int nW = a.ny * a.nx;
  const long items = (long)a.planes * a.chunks;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const int p = (int)(item / a.chunks), j = (int)(item - (long)p * a.chunks);  // window plane (b * nW + k) * C + c, pass within it
    const int bk = p / a.C, c = p - bk * a.C;
    const int b = bk / nW, k = bk - b * nW;
    const int ky = k / a.nx, kx = k - ky * a.nx;
    const int u = j * a.rpw + r_local;
    if (r_local >= a.rpw || u >= a.S) continue;
    int y = a.oy[ky] + u;
    if (y >= a.H) y -= a.H;  // only under wrap: the launcher has checked oy + S <= H otherwise
    const float* src = full + ((long)(b * a.C + c) * a.H + y) * a.W;
    float* dst = win + ((long)p * a.S + u) * a.S;
    const float wy = a.ay ? a.ay[ky * a.S + u] : 1.f;
    for (int un = u0; un < a.upr; un += 256) {
      const int v = un * V;
      int x = a.ox[kx] + v;
      if (x >= a.W) x -= a.W;
      float f[V];
      load<V>(src + x, f);
      if (a.ay) {  // the tables come as a pair
        float wx[V];
        load<V>(a.ax + kx * a.S + v, wx);
#pragma unroll
        for (int e = 0; e < V; ++e) f[e] = (wy * wx[e]) * f[e];
      }
      store<V>(dst + v, f);
    }
  }
}

template <int V>
__global__ __launch_bounds__(256) void window_merge_kernel(const float* __restrict__ win, float* __restrict__ full, WindowArgs a, int accumulate) {
  int r_local, u0;
  thread_slot(a, r_local, u0);
  const int nW = a.ny * a.nx;
  const long SS = (long)a.S * a.S;
  const long items = (long)a.planes * a.chunks;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const int p = (int)(item / a.chunks), j = (int)(item - (long)p * a.chunks);  // frame plane b * C + c, pass within it
    const int b = p / a.C, c = p - b * a.C;
    const int y = j * a.rpw + r_local;
    if (r_local >= a.rpw || y >= a.H) continue;
    float* dst = full + ((long)p * a.H + y) * a.W;
    for (int un = u0; un < a.upr; un += 256) {
      const int x = un * V;
      float acc[V];
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = -0.f;  // -0 + t == t for every t, signed zeros included: a single window of weight one keeps its bits
      for (int ky = 0; ky < a.ny; ++ky) {
        int u = y - a.oy[ky];
        if (u < 0 && (a.wrap & 2)) u += a.H;
        if (u < 0 || u >= a.S) continue;
        const float wy = a.ay ? a.ay[ky * a.S + u] : 1.f;
        for (int kx = 0; kx < a.nx; ++kx) {
          int v = x - a.ox[kx];
          if (v < 0 && (a.wrap & 1)) v += a.W;
          if (v < 0 || v >= a.S) continue;
          float t[V];
          load<V>(win + ((long)((b * nW + ky * a.nx + kx) * a.C + c)) * SS + (long)u * a.S + v, t);
          if (a.ay) {
            float wx[V];
            load<V>(a.ax + kx * a.S + v, wx);
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] += (wy * wx[e]) * t[e];
          } else {
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] += t[e];
          }
        }
      }
      if (accumulate) {
        float f[V];
        load<V>(dst + x, f);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] += f[e];
      }
      store<V>(dst + x, acc);
    }
  }
}

// One axis of the plan: extent L, n origins o, window side S, wrapping or not.  Returns null or what is wrong with it.
const char* check_axis(const int* o, int n, int L, int S, bool wrap) {
  if (n < 1 || n > kMaxWin) return "between 1 and 16 windows per axis";
  if (L % 8 || S > L) return "the frame sides must be multiples of 8 and at least the window side";
  std::vector<char> covered(L / 8, 0);  // per block of 8 pixels
  for (int k = 0; k < n; ++k) {
    if (o[k] % 8) return "window origins must be multiples of 8";
    if (o[k] < 0 || o[k] >= L) return "a window origin lies outside the frame";
    if (!wrap && o[k] + S > L) return "a window runs over an edge that does not wrap";
    for (int q = 0; q < S / 8; ++q) covered[(o[k] / 8 + q) % (L / 8)] = 1;
  }
  for (char q : covered)
    if (!q) return "the windows do not cover the frame";
  return nullptr;
}

struct Plan {
  WindowArgs a;
  bool vec;
  int grid;
};

int make_plan(cgd_ctx* ctx, const char* what, const float* full, const float* win, const int* oy, int ny, const int* ox, int nx,
              const float* ay, const float* ax, int B, int C, int H, int W, int S, int wrap, bool merge, Plan& pl) {
  auto fail = [&](const char* why) { return std::string(what) + ": " + why; };
  if (!full || !win || !oy || !ox) CGD_FAIL(ctx, fail("full, win and the window origins are required"));
  if ((ay != nullptr) != (ax != nullptr)) CGD_FAIL(ctx, fail("the weight tables come as a pair (both or none)"));
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || S <= 0) CGD_FAIL(ctx, fail("empty shape"));
  if (wrap & ~3) CGD_FAIL(ctx, fail("wrap is bit 0 (x) | bit 1 (y)"));
  if (S % 8) CGD_FAIL(ctx, fail("the window side must be a multiple of 8"));
  if ((long)H * W > INT32_MAX || (long)S * S > INT32_MAX) CGD_FAIL(ctx, fail("a plane exceeds 2^31 - 1 elements"));
  if (const char* why = check_axis(oy, ny, H, S, wrap & 2)) CGD_FAIL(ctx, fail(why));
  if (const char* why = check_axis(ox, nx, W, S, wrap & 1)) CGD_FAIL(ctx, fail(why));
  const long nW = (long)ny * nx;
  if ((long)B * nW * C > INT32_MAX / 256) CGD_FAIL(ctx, fail("too many window planes"));
  WindowArgs& a = pl.a;
  a.ay = ay;
  a.ax = ax;
  for (int k = 0; k < kMaxWin; ++k) {
    a.oy[k] = k < ny ? oy[k] : 0;
    a.ox[k] = k < nx ? ox[k] : 0;
  }
  a.ny = ny; a.nx = nx; a.C = C; a.H = H; a.W = W; a.S = S; a.wrap = wrap;
  pl.vec = aligned16(full) && aligned16(win) && aligned16(ay) && aligned16(ax);
  const int row = merge ? W : S, rows = merge ? H : S;  // the walked tensor: the one that is written
  a.planes = (int)(merge ? (long)B * C : (long)B * nW * C);
  a.upr = pl.vec ? row / 4 : row;
  a.rpw = a.upr >= 256 ? 1 : std::min(256 / a.upr, rows);
  a.chunks = cdiv(rows, a.rpw);
  // memory-bound streaming: at most 8 workgroups per CU, the rest of the passes by grid stride
  pl.grid = (int)std::min((long)a.planes * a.chunks, (long)ctx->num_cu * 8);
  return 0;
}

}  // namespace

int cgd_launch_window_gather(cgd_ctx* ctx, const float* full, float* win, const int* oy, int ny, const int* ox, int nx, const float* ay,
                             const float* ax, int B, int C, int H, int W, int S, int wrap, hipStream_t s) {
  Plan pl;
  CGD_TRY(make_plan(ctx, "window gather", full, win, oy, ny, ox, nx, ay, ax, B, C, H, W, S, wrap, false, pl));
  if (pl.vec)
    CGD_LAUNCH(window_gather_kernel<4>, dim3(pl.grid), dim3(256), 0, s, full, win, pl.a);
  else
    CGD_LAUNCH(window_gather_kernel<1>, dim3(pl.grid), dim3(256), 0, s, full, win, pl.a);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

int cgd_launch_window_merge(cgd_ctx* ctx, const float* win, float* full, const int* oy, int ny, const int* ox, int nx, const float* ay,
                            const float* ax, int B, int C, int H, int W, int S, int wrap, int accumulate, hipStream_t s) {
  Plan pl;
  CGD_TRY(make_plan(ctx, "window merge", full, win, oy, ny, ox, nx, ay, ax, B, C, H, W, S, wrap, true, pl));
  if (pl.vec)
    CGD_LAUNCH(window_merge_kernel<4>, dim3(pl.grid), dim3(256), 0, s, win, full, pl.a, accumulate != 0);
  else
    CGD_LAUNCH(window_merge_kernel<1>, dim3(pl.grid), dim3(256), 0, s, win, full, pl.a, accumulate != 0);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
