// Fused optimizer-update CDNA4 kernels: AdamW and SGD(momentum).
//
// The reference's update math is 7+ separate torch kernel launches per
// parameter (/root/reference/tiny_deepspeed/core/optim/adamw.py:32-59,
// sgd.py:28-46). Here one launch updates every parameter in a single HBM
// pass (fp32 state, fp32 master copy for bf16 params): a per-parameter
// python loop costs ~200 launches x 15us per step (measured). The
// reference's per-parameter step-count bug is fixed: `step` is the global
// 1-based optimizer step.
#include "common.h"
#include "launchers.h"
#include "optim_desc.h"

namespace tdsa {

// One chunk [start, end) of one tensor under `rule`, with S fp32 state
// streams `st`. 4 elements per lane with EXPLICIT dwordx4/dwordx2 accesses:
// the fp32 state (m, v, buf, master) dominates the 10+ GB/step traffic and
// the element-wise form compiled to scalar flat_load_dword (checked in the
// .s — the unroll never re-vectorized). HASM as a template so the master
// loads/stores are unconditional in the fast path.
//
// HASG: every gradient element is multiplied by `gs` (the clip coefficient of
// a max_grad_norm step) in fp32 before the rule sees it. A template flag and
// not a multiply by 1.0f, so that the unscaled instantiations keep the
// instruction stream they had before the scale existed.
template <bool HASG>
DEV_INLINE float scaled(float g, float gs) {
#pragma clang fp contract(off)
  return HASG ? g * gs : g;
}

template <int S, bool HASM, bool HASG, typename Rule, typename PT, typename GT>
DEV_INLINE void update_span(const Rule& rule, PT* p, const GT* g,
                            const typename Rule::Desc& d, float* const* st,
                            long long start, long long end, float gs) {
  // params/grads 4 wide in either dtype, next to the fp32 state vectors
  typedef Vec<PT, 4> PVec;
  typedef Vec<GT, 4> GVec;
  typedef typename PVec::V PV;
  typedef typename GVec::V GV;
  float* const master = d.master;
  const long long n4 = (end - start) / 4;
  for (long long q = threadIdx.x; q < n4; q += blockDim.x) {
    const long long i = start + q * 4;
    const GV gv = *reinterpret_cast<const GV*>(g + i);
    f32x4 sv[S + 1];  // +1: S may be 0
#pragma unroll
    for (int j = 0; j < S; ++j)
      sv[j] = *reinterpret_cast<const f32x4*>(st[j] + i);
    f32x4 pv;
    if (HASM) {
      pv = *reinterpret_cast<const f32x4*>(master + i);
    } else {
      const PV praw = *reinterpret_cast<const PV*>(p + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) pv[k] = PVec::get(praw, k);
    }
    PV pout;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float s[S + 1];
#pragma unroll
      for (int j = 0; j < S; ++j) s[j] = sv[j][k];
      pv[k] = rule.template elem<S>(d, scaled<HASG>(GVec::get(gv, k), gs),
                                    pv[k], s);
#pragma unroll
      for (int j = 0; j < S; ++j) sv[j][k] = s[j];
      PVec::set(pout, k, pv[k]);
    }
#pragma unroll
    for (int j = 0; j < S; ++j) *reinterpret_cast<f32x4*>(st[j] + i) = sv[j];
    if (HASM) *reinterpret_cast<f32x4*>(master + i) = pv;
    *reinterpret_cast<PV*>(p + i) = pout;
  }
  for (long long i = start + n4 * 4 + threadIdx.x; i < end; i += blockDim.x) {
    float s[S + 1];
#pragma unroll
    for (int j = 0; j < S; ++j) s[j] = st[j][i];
    const float pk = rule.template elem<S>(
        d, scaled<HASG>((float)g[i], gs), HASM ? master[i] : (float)p[i], s);
#pragma unroll
    for (int j = 0; j < S; ++j) st[j][i] = s[j];
    if (HASM) master[i] = pk;
    p[i] = (PT)pk;
  }
}

// ---- update rules ----------------------------------------------------------
// A rule is the kernel argument of optim_multi_kernel: the hyper-parameters,
// elem() — the per-element math on registers, which updates the element's S
// fp32 state values `s` in place and returns the new parameter — and
// chunk(), which picks the compile-time update_span variant for one tensor.
//
// elem() spells out its roundings (contraction off, explicit fmaf) so that
// the vector body and the scalar tail of every dtype variant round alike,
// whatever the vectorizer makes of the surrounding code.
template <bool AMS>
struct AdamW {
  typedef AdamTensorDesc Desc;
  float lr, b1, b2, eps, wd, inv_bc1, inv_bc2;

  // s = {m, v} or, with amsgrad, {m, v, vmax}
  template <int S>
  DEV_INLINE float elem(const Desc&, float g, float p, float* s) const {
#pragma clang fp contract(off)
    const float m = s[0] = fmaf(1.0f - b1, g, s[0] * b1);
    float v = s[1] = fmaf(s[1], b2, (1.0f - b2) * g * g);
    if (AMS) v = s[2] = fmaxf(s[2], v);
    const float step = lr * inv_bc1 * m / (sqrtf(v * inv_bc2) + eps);
    return fmaf(p, fmaf(-lr, wd, 1.0f), -step);
  }

  template <bool HASG, typename PT, typename GT>
  DEV_INLINE void chunk(PT* p, const GT* g, const Desc& d, long long start,
                        long long end, float gs) const {
    constexpr int S = AMS ? 3 : 2;
    float* const st[3] = {d.m, d.v, d.vmax};
    if (d.master)
      update_span<S, true, HASG>(*this, p, g, d, st, start, end, gs);
    else
      update_span<S, false, HASG>(*this, p, g, d, st, start, end, gs);
  }
};

struct Sgd {
  typedef SgdTensorDesc Desc;
  float lr, momentum, dampening, wd;
  int nesterov, maximize;

  // s = {buf} with momentum (S = 1), empty without
  template <int S>
  DEV_INLINE float elem(const Desc& d, float g, float p, float* s) const {
#pragma clang fp contract(off)
    if (maximize) g = -g;
    if (wd != 0.0f) g = fmaf(wd, p, g);
    if (S) {
      const float b = d.first ? g : s[0] * momentum + (1.0f - dampening) * g;
      s[0] = b;
      g = nesterov ? fmaf(momentum, b, g) : b;
    }
    return fmaf(-lr, g, p);
  }

  template <bool HASG, typename PT, typename GT>
  DEV_INLINE void chunk(PT* p, const GT* g, const Desc& d, long long start,
                        long long end, float gs) const {
    float* const st[1] = {d.buf};
    if (d.buf && d.master)
      update_span<1, true, HASG>(*this, p, g, d, st, start, end, gs);
    else if (d.buf)
      update_span<1, false, HASG>(*this, p, g, d, st, start, end, gs);
    else if (d.master)
      update_span<0, true, HASG>(*this, p, g, d, st, start, end, gs);
    else
      update_span<0, false, HASG>(*this, p, g, d, st, start, end, gs);
  }
};

// The chunk loop and the (param, grad) dtype ladder of both optimizers.
// HASG: gscale points at the gradient scale, which each lane reads once,
// before its chunk loop; without it gscale is not touched.
template <typename Rule, bool HASG>
__global__ void optim_multi_kernel(
    const typename Rule::Desc* __restrict__ descs,
    const ChunkRef* __restrict__ chunks, int nchunks, int chunk_elems,
    Rule rule, const float* __restrict__ gscale) {
  const float gs = HASG ? *gscale : 1.0f;
  for (int cid = blockIdx.x; cid < nchunks; cid += gridDim.x) {
    const ChunkRef ch = chunks[cid];
    const typename Rule::Desc d = descs[ch.tensor];
    const long long start = (long long)ch.chunk * chunk_elems;
    const long long end = min(d.numel, start + chunk_elems);
    if (d.param_bf16 && d.grad_bf16)
      rule.template chunk<HASG>((bf16*)d.p, (const bf16*)d.g, d, start, end,
                                gs);
    else if (d.param_bf16)
      rule.template chunk<HASG>((bf16*)d.p, (const float*)d.g, d, start, end,
                                gs);
    else if (d.grad_bf16)
      rule.template chunk<HASG>((float*)d.p, (const bf16*)d.g, d, start, end,
                                gs);
    else
      rule.template chunk<HASG>((float*)d.p, (const float*)d.g, d, start, end,
                                gs);
  }
}

// Grid sizing, blob split and launch.
template <typename Rule>
hipError_t launch_multi(const Rule& rule, const void* blob, int ndescs,
                        int nchunks, const float* gscale, hipStream_t stream) {
  const typename Rule::Desc* descs = (const typename Rule::Desc*)blob;
  const ChunkRef* chunks = (const ChunkRef*)(descs + ndescs);
  int grid = nchunks < 2048 ? nchunks : 2048;
  if (grid < 1) grid = 1;
  if (gscale)
    hipLaunchKernelGGL((optim_multi_kernel<Rule, true>), dim3(grid), dim3(256),
                       0, stream, descs, chunks, nchunks, kOptimChunkElems,
                       rule, gscale);
  else
    hipLaunchKernelGGL((optim_multi_kernel<Rule, false>), dim3(grid),
                       dim3(256), 0, stream, descs, chunks, nchunks,
                       kOptimChunkElems, rule, gscale);
  return hipGetLastError();
}

}  // namespace tdsa

using namespace tdsa;

extern "C" {

// amsgrad: every descriptor carries a vmax.
hipError_t tdsa_adamw_multi(const void* blob, int ndescs, int nchunks,
                            int amsgrad, float lr, float b1, float b2,
                            float eps, float wd, long long step,
                            const float* gscale, hipStream_t stream) {
  const float inv_bc1 = 1.0f / (1.0f - powf(b1, (float)step));
  const float inv_bc2 = 1.0f / (1.0f - powf(b2, (float)step));
  if (amsgrad)
    return launch_multi(AdamW<true>{lr, b1, b2, eps, wd, inv_bc1, inv_bc2},
                        blob, ndescs, nchunks, gscale, stream);
  return launch_multi(AdamW<false>{lr, b1, b2, eps, wd, inv_bc1, inv_bc2},
                      blob, ndescs, nchunks, gscale, stream);
}

hipError_t tdsa_sgd_multi(const void* blob, int ndescs, int nchunks, float lr,
                          float momentum, float dampening, float wd,
                          int nesterov, int maximize, const float* gscale,
                          hipStream_t stream) {
  return launch_multi(Sgd{lr, momentum, dampening, wd, nesterov, maximize},
                      blob, ndescs, nchunks, gscale, stream);
}

}  // extern "C"
