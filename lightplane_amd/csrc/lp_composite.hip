// lp_composite.hip -- the ray march as two stand-alone ops (include/lightplane_hip_samples.h): where the Renderer places its samples
// (ray_samples_fwd / _bwd) and its emission-absorption integral over per-sample opacities and features (composite_fwd / _bwd).
// fp32, no atomics, no workspace, no host synchronisation.  Arguments are checked by lp_api.hip.
//
// Compositing: one wavefront (= one workgroup) per ray, lanes over samples in chunks of 64.  The prefix of od = opacity * delta and the
// reverse suffix of w * v are wave scans with a carry between chunks.  The ray's S * C features are one contiguous run: a lane owns one
// channel unit (V = 4 floats where C % 4 == 0, one float otherwise), floor(64 / CV) samples of CV = C / V units go through the wave per
// load instruction, and lanes of equal unit are folded through LDS at the end.  CV > 64 (C = 65 .. 127, not a multiple of 4): two units
// per lane, one sample per step.
#include "lp_host.h"
#include "lp_rows.h"
#include "lp_wave.h"

namespace lp {

namespace {

constexpr int RS_THREADS = 256;  // ray_samples_fwd: samples per workgroup; ray_samples_bwd: 4 rays per workgroup
constexpr int CB_SUPER = 512;    // composite_bwd: chunks whose starting -log T are kept in LDS at a time (32 768 samples)

struct RsArgs {
  LpRays rays;
  LpMarch march;
  float *points, *depths, *deltas;
  const float *g_points, *g_depths, *g_deltas;
  float *g_origins, *g_directions, *g_near, *g_far;
};

// grid_idx is not read (it may be NULL): the ray's geometry only
LP_DEV Ray load_ray_geometry(const LpRays& r, int64_t i) {
  Ray q;
  load_ray_line(r.origins, r.directions, i, q);
  q.near_t = r.near_t[i];
  q.far_t = r.far_t[i];
  q.b = 0;
  return q;
}

// One lane per sample, n_items = n_rays * S_tot < 2^31 of them; the points leave through LDS so that a workgroup's 3 * 256 floats are
// stored as one contiguous run.
__global__ __launch_bounds__(RS_THREADS) void ray_samples_fwd(RsArgs a, int S_tot, int64_t n_items) {
  __shared__ float pts[3 * RS_THREADS];
  const int t = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * RS_THREADS;
  const int64_t i = i0 + t;
  if (i < n_items) {
    const int64_t r = (unsigned)i / (unsigned)S_tot;  // (n_items < 2^31)
    const int s = (int)(i - r * S_tot);
    const Ray q = load_ray_geometry(a.rays, r);
    const float depth = sample_depth(s, a.march, q.near_t, q.far_t);
    float x, y, z;
    sample_point(q, depth, false, x, y, z);
    a.depths[i] = depth;
    a.deltas[i] = sample_delta(s, a.march, q.near_t, q.far_t, depth);
    pts[3 * t + 0] = x;
    pts[3 * t + 1] = y;
    pts[3 * t + 2] = z;
  }
  __syncthreads();
  const int64_t left = n_items - i0;
  const int n = 3 * (int)(left < RS_THREADS ? left : RS_THREADS);
  for (int j = t; j < n; j += RS_THREADS) a.points[3 * i0 + j] = pts[j];
}

// One wavefront per ray.  Everything is linear in near / far: depth_i = near + l_i (far - near) (i < S), far c_k (i = S + k),
// delta_0 = (far - near) / (S - 1) or the constant 1, delta_i = depth_i - depth_{i-1}.  grad_points is read as the contiguous run of
// 3 S_tot floats it is: element e belongs to sample e / 3, component e % 3.
__global__ __launch_bounds__(RS_THREADS) void ray_samples_bwd(RsArgs a, int S_tot) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (RS_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= a.rays.n_rays) return;  // (wave-uniform)
  const Ray q = load_ray_geometry(a.rays, r);
  const LpMarch& m = a.march;
  const int S = m.num_samples;
  float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f, d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, g_near = 0.0f, g_far = 0.0f;
  // the gradient g of depth_s, passed on to near and far
  auto depth_grad = [&](int s, float g) {
    if (s < S) {
      const float l = lin01(s, S);
      g_near += (1.0f - l) * g;
      g_far += l * g;
    } else {
      g_far += inf_scale(s - S, m) * g;
    }
  };
  const int64_t base = r * S_tot;
  if (a.g_points) {
    const float* gp = a.g_points + 3 * base;
    for (int64_t e = lane; e < 3 * (int64_t)S_tot; e += 64) {
      const int s = (int)(e / 3), c = (int)(e - 3 * (int64_t)s);
      const float v = gp[e];
      const float vd = v * sample_depth(s, m, q.near_t, q.far_t);
      o0 += c == 0 ? v : 0.0f;
      o1 += c == 1 ? v : 0.0f;
      o2 += c == 2 ? v : 0.0f;
      d0 += c == 0 ? vd : 0.0f;
      d1 += c == 1 ? vd : 0.0f;
      d2 += c == 2 ? vd : 0.0f;
      depth_grad(s, v * (c == 0 ? q.dx : c == 1 ? q.dy : q.dz));
    }
  }
  if (a.g_depths)
    for (int s = lane; s < S_tot; s += 64) depth_grad(s, a.g_depths[base + s]);
  if (a.g_deltas)
    for (int s = lane; s < S_tot; s += 64) {
      const float g = a.g_deltas[base + s];
      if (s > 0) {
        depth_grad(s, g);
        depth_grad(s - 1, -g);
      } else if (S > 1) {
        const float gs = g / (float)(S - 1);
        g_far += gs;
        g_near -= gs;
      }
    }
  o0 = wave_sum(o0), o1 = wave_sum(o1), o2 = wave_sum(o2);
  d0 = wave_sum(d0), d1 = wave_sum(d1), d2 = wave_sum(d2);
  g_near = wave_sum(g_near), g_far = wave_sum(g_far);
  if (lane == 0) {
    if (a.g_origins) a.g_origins[3 * r + 0] = o0, a.g_origins[3 * r + 1] = o1, a.g_origins[3 * r + 2] = o2;
    if (a.g_directions) a.g_directions[3 * r + 0] = d0, a.g_directions[3 * r + 1] = d1, a.g_directions[3 * r + 2] = d2;
    if (a.g_near) a.g_near[r] = g_near;
    if (a.g_far) a.g_far[r] = g_far;
  }
}

struct CpArgs {
  const float *opacity, *features, *depths, *deltas;
  int64_t n_rays;
  int S, C;
  float *ray_length, *nlt, *feature, *weights;
  const float *g_len, *g_nlt, *g_feat, *g_w;
  float *g_opacity, *g_features, *g_depths, *g_deltas;
};

// How the lanes of a wave share the features of a ray: which channel unit(s) a lane owns and which of the G samples of a step.
template <int V, int NB>
struct FeatLanes {
  int CV, G, A, u0, q;
  LP_DEV FeatLanes(int C, int lane) {
    CV = C / V;
    if (NB == 2) {
      G = 1, A = 64, u0 = lane, q = 0;
    } else {
      G = CV > 0 ? 64 / CV : 1;
      A = G * CV;
      u0 = CV > 0 ? lane % CV : 0;
      q = CV > 0 ? lane / CV : 0;
    }
  }
};

// dynamic LDS: wl[64] | fold[NB * 64 * V]
template <int V, int NB>
__global__ __launch_bounds__(64) void composite_fwd(CpArgs a) {
  extern __shared__ float4 smem4[];
  float* wl = reinterpret_cast<float*>(smem4);
  float* fold = wl + 64;
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  const int S = a.S, C = a.C;
  const bool has_feat = C > 0;
  const FeatLanes<V, NB> fl(C, lane);
  const int64_t base = r * S;
  float carry = 0.0f, len = 0.0f;
  float acc[NB][V];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int v = 0; v < V; ++v) acc[b][v] = 0.0f;

  for (int64_t s0 = 0; s0 < S; s0 += 64) {
    const int64_t s = s0 + lane;
    const bool in = s < S;
    const float o = in ? a.opacity[base + s] : 0.0f;
    const float dl = in ? a.deltas[base + s] : 0.0f;
    const float dp = in ? a.depths[base + s] : 0.0f;
    const float od = o * dl;
    const float incl = wave_scan(od, lane);
    const float up = __shfl_up(incl, 1, 64);
    const float nlt = carry + (lane > 0 ? up : 0.0f);  // -log T in front of the sample
    const float w = expf(-nlt) * (-expm1f(-od));
    len += w * dp;
    if (a.weights && in) a.weights[base + s] = w;
    carry += __shfl(incl, 63, 64);
    if (has_feat) {
      wl[lane] = w;
      __syncthreads();
      const int n = S - s0 < 64 ? (int)(S - s0) : 64;
      const float* f0 = a.features + (base + s0) * C;
      for (int sl0 = 0; sl0 < n; sl0 += fl.G) {
        const int sl = sl0 + fl.q;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const int u = fl.u0 + 64 * b;
          if (lane < fl.A && sl < n && u < fl.CV) {
            const Vec<V> f = vec_load<V>(f0 + (int64_t)sl * C + u * V);
            const float ws = wl[sl];
#pragma unroll
            for (int v = 0; v < V; ++v) acc[b][v] = fmaf(ws, f.v[v], acc[b][v]);
          }
        }
      }
      __syncthreads();
    }
  }
  len = wave_sum(len);
  if (lane == 0) {
    a.ray_length[r] = len;
    a.nlt[r] = carry;
  }
  if (has_feat) {
    // lanes of equal unit, in the order of their samples
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int v = 0; v < V; ++v) fold[(b * 64 + lane) * V + v] = acc[b][v];
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int u = lane + 64 * b;
      if (lane < (NB == 2 ? 64 : fl.CV) && u < fl.CV) {
        Vec<V> sum;
#pragma unroll
        for (int v = 0; v < V; ++v) sum.v[v] = 0.0f;
        for (int g = 0; g < fl.G; ++g)
#pragma unroll
          for (int v = 0; v < V; ++v) sum.v[v] += fold[(b * 64 + g * fl.CV + lane) * V + v];
        vec_store<V>(a.feature + r * C + u * V, sum);
      }
    }
  }
}

// dynamic LDS: wl[64] | start[CB_SUPER] | P[64 * stride], stride = CV | 1
// Pass A walks the chunks near -> far and keeps the -log T every chunk starts from; pass B walks them far -> near with the reverse
// suffix of w v.  A ray of more than CB_SUPER chunks is done in super-blocks from the far end, each with its own pass A from the start
// of the ray (opacity and deltas are then read more than twice: 32 768 samples per ray and more).
template <int V, int NB>
__global__ __launch_bounds__(64) void composite_bwd(CpArgs a) {
  extern __shared__ float4 smem4[];
  float* wl = reinterpret_cast<float*>(smem4);
  float* start = wl + 64;
  float* P = start + CB_SUPER;
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  const int S = a.S, C = a.C;
  const FeatLanes<V, NB> fl(C, lane);
  const int stride = fl.CV | 1;
  const int64_t base = r * S;
  const float gl = a.g_len ? a.g_len[r] : 0.0f;
  const float gn = a.g_nlt ? a.g_nlt[r] : 0.0f;
  const bool need_od = a.g_opacity || a.g_deltas;
  const bool need_dot = C > 0 && a.g_feat && need_od;
  const bool feat_loop = C > 0 && (need_dot || a.g_features);
  float gf[NB][V];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int u = fl.u0 + 64 * b;
#pragma unroll
    for (int v = 0; v < V; ++v) gf[b][v] = (a.g_feat && u < fl.CV) ? a.g_feat[r * C + u * V + v] : 0.0f;
  }
  const int n_chunks = (int)(((int64_t)S + 63) / 64);
  float rev = 0.0f;  // sum of w v over the chunks behind
  for (int k_end = n_chunks; k_end > 0; k_end -= CB_SUPER) {
    const int k_begin = k_end > CB_SUPER ? k_end - CB_SUPER : 0;
    float carry = 0.0f;
    for (int k = 0; k < k_end; ++k) {
      const int64_t s = (int64_t)k * 64 + lane;
      const bool in = s < S;
      const float od = in ? a.opacity[base + s] * a.deltas[base + s] : 0.0f;
      if (k >= k_begin && lane == 0) start[k - k_begin] = carry;
      carry += __shfl(wave_scan(od, lane), 63, 64);
    }
    __syncthreads();
    for (int k = k_end - 1; k >= k_begin; --k) {
      const int64_t s0 = (int64_t)k * 64, s = s0 + lane;
      const bool in = s < S;
      const float c0 = start[k - k_begin];
      const float o = in ? a.opacity[base + s] : 0.0f;
      const float dl = in ? a.deltas[base + s] : 0.0f;
      const float dp = in ? a.depths[base + s] : 0.0f;
      const float gw = (in && a.g_w) ? a.g_w[base + s] : 0.0f;
      const float od = o * dl;
      const float incl = wave_scan(od, lane);
      const float up = __shfl_up(incl, 1, 64);
      const float t_next = expf(-(c0 + incl));  // T behind the sample
      const float w = expf(-(c0 + (lane > 0 ? up : 0.0f))) * (-expm1f(-od));
      float dot = 0.0f;
      if (feat_loop) {
        wl[lane] = w;
        __syncthreads();
        const int n = S - s0 < 64 ? (int)(S - s0) : 64;
        const int64_t f0 = (base + s0) * C;
        for (int sl0 = 0; sl0 < n; sl0 += fl.G) {
          const int sl = sl0 + fl.q;
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            const int u = fl.u0 + 64 * b;
            if (lane < fl.A && sl < n && u < fl.CV) {
              const int64_t at = f0 + (int64_t)sl * C + u * V;
              if (need_dot) {
                const Vec<V> f = vec_load<V>(a.features + at);
                float p = 0.0f;
#pragma unroll
                for (int v = 0; v < V; ++v) p = fmaf(f.v[v], gf[b][v], p);
                P[sl * stride + u] = p;
              }
              if (a.g_features) {
                const float ws = wl[sl];
                Vec<V> g;
#pragma unroll
                for (int v = 0; v < V; ++v) g.v[v] = ws * gf[b][v];
                vec_store<V>(a.g_features + at, g);
              }
            }
          }
        }
        __syncthreads();
        if (need_dot && lane < n)
          for (int u = 0; u < fl.CV; ++u) dot += P[lane * stride + u];
      }
      const float v = gl * dp + dot + gw;
      const float rincl = wave_rscan(w * v, lane);
      const float down = __shfl_down(rincl, 1, 64);
      const float behind = rev + (lane < 63 ? down : 0.0f);
      const float d_od = t_next * v - behind + gn;
      if (in) {
        if (a.g_opacity) a.g_opacity[base + s] = d_od * dl;
        if (a.g_deltas) a.g_deltas[base + s] = d_od * o;
        if (a.g_depths) a.g_depths[base + s] = gl * w;
      }
      rev += __shfl(rincl, 0, 64);
    }
    __syncthreads();
  }
}

template <int V, int NB>
void composite_launch_as(const CpArgs& s, bool backward, hipStream_t stream) {
  const int CV = s.C / V;
  // (one workgroup per ray: check_point_batch of lp_api.hip keeps n_rays * n_samples, hence n_rays, below 2^31)
  if (backward) {
    const size_t lds = sizeof(float) * (size_t)(64 + CB_SUPER + 64 * (CV | 1));
    hipLaunchKernelGGL((composite_bwd<V, NB>), dim3((unsigned)s.n_rays), dim3(64), lds, stream, s);
  } else {
    const size_t lds = sizeof(float) * (size_t)(64 + NB * 64 * V);
    hipLaunchKernelGGL((composite_fwd<V, NB>), dim3((unsigned)s.n_rays), dim3(64), lds, stream, s);
  }
}

}  // namespace

// `a` checked by lp_api.hip: n_rays > 0, n_rays * S_tot < 2^31
int ray_samples_launch(const LpRaySamplesArgs& a, bool backward, hipStream_t stream) {
  RsArgs s;
  s.rays = a.rays;
  s.march = a.march;
  s.points = a.points, s.depths = a.depths, s.deltas = a.deltas;
  s.g_points = a.grad_points, s.g_depths = a.grad_depths, s.g_deltas = a.grad_deltas;
  s.g_origins = a.grad_origins, s.g_directions = a.grad_directions, s.g_near = a.grad_near, s.g_far = a.grad_far;
  const int S_tot = a.march.num_samples + a.march.num_samples_inf;
  unsigned blocks;
  if (backward) {
    if (!s.g_origins && !s.g_directions && !s.g_near && !s.g_far) return LP_OK;
    if (int rc = launch_blocks("lp_ray_samples_backward", a.rays.n_rays, RS_THREADS / 64, blocks)) return rc;
    hipLaunchKernelGGL(ray_samples_bwd, dim3(blocks), dim3(RS_THREADS), 0, stream, s, S_tot);
    return check_launch("ray_samples_bwd");
  }
  const int64_t n_items = a.rays.n_rays * S_tot;
  if (int rc = launch_blocks("lp_ray_samples_forward", n_items, RS_THREADS, blocks)) return rc;
  hipLaunchKernelGGL(ray_samples_fwd, dim3(blocks), dim3(RS_THREADS), 0, stream, s, S_tot, n_items);
  return check_launch("ray_samples_fwd");
}

// `a` checked by lp_api.hip: n_rays > 0, n_rays * n_samples < 2^31, 0 <= channels <= LP_MAX_WIDTH
int composite_launch(const LpCompositeArgs& a, bool backward, hipStream_t stream) {
  CpArgs s;
  s.opacity = a.opacity, s.features = a.features, s.depths = a.depths, s.deltas = a.deltas;
  s.n_rays = a.n_rays, s.S = a.n_samples, s.C = a.channels;
  s.ray_length = a.ray_length, s.nlt = a.neg_log_t, s.feature = a.feature, s.weights = a.weights;
  s.g_len = a.grad_ray_length, s.g_nlt = a.grad_neg_log_t, s.g_feat = a.grad_feature, s.g_w = a.grad_weights;
  s.g_opacity = a.grad_opacity, s.g_features = a.grad_features, s.g_depths = a.grad_depths, s.g_deltas = a.grad_deltas;
  if (backward && !s.g_opacity && !s.g_features && !s.g_depths && !s.g_deltas) return LP_OK;
  if (s.C % 4 == 0) composite_launch_as<4, 1>(s, backward, stream);  // (C = 0: no unit, no lane reads a feature)
  else if (s.C <= 64) composite_launch_as<1, 1>(s, backward, stream);
  else composite_launch_as<1, 2>(s, backward, stream);
  return check_launch(backward ? "composite_bwd" : "composite_fwd");
}

}  // namespace lp
