// Python bindings for the tiny_deepspeed_amd CDNA4 kernel extension (_C).
//
// Host-side glue only: shape/dtype checks, output allocation, stream lookup.
// All device code lives in csrc/kernels/*.hip (pure HIP, no torch headers).
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <hip/hip_runtime_api.h>

#include "kernels/launchers.h"
#include "kernels/optim_desc.h"

#include <array>
#include <climits>
#include <cstring>
#include <vector>

namespace {

void check_hip(hipError_t err, const char* what) {
  TORCH_CHECK(err == hipSuccess, what, ": ", hipGetErrorString(err));
}

int dtype_flag(const at::Tensor& t) {
  if (t.scalar_type() == at::kBFloat16) return 1;
  if (t.scalar_type() == at::kFloat) return 0;
  TORCH_CHECK(false, "expected float32 or bfloat16, got ", t.scalar_type());
  return -1;
}

hipStream_t cur_stream() {
  return (hipStream_t)at::cuda::getCurrentCUDAStream().stream();
}

// ---- argument checks of the non-attention, non-optimizer bindings ---------
// One argument of a call; an absent optional one is skipped. Every argument
// must be on the first one's GPU. dtype: the one it must have; none means
// the first argument's, which itself must be float32 or bfloat16. numel: its
// element count (kAny: not checked). strided: the binding makes its own
// contiguous copy, so any layout is accepted.
constexpr int64_t kAny = -1;
struct Arg {
  const char* name;
  c10::optional<at::Tensor> t;
  c10::optional<at::ScalarType> dtype;
  int64_t numel;
  bool strided = false;
};

// Checks all of `args` in one pass, before anything is allocated or
// launched, and returns the first argument's dtype flag.
int check_call(const char* op, std::initializer_list<Arg> args) {
  const at::Tensor& first = *args.begin()->t;
  for (const Arg& a : args) {
    if (!a.t.has_value()) continue;
    const at::Tensor& t = *a.t;
    TORCH_CHECK(t.is_cuda(), op, ": ", a.name, " must be on GPU");
    TORCH_CHECK(t.device() == first.device(), op, ": ", a.name, " is on ",
                t.device(), ", ", args.begin()->name, " on ", first.device());
    TORCH_CHECK(a.strided || t.is_contiguous(), op, ": ", a.name,
                " must be contiguous");
    const at::ScalarType want = a.dtype.value_or(first.scalar_type());
    TORCH_CHECK(t.scalar_type() == want, op, ": ", a.name, " must be ", want,
                ", got ", t.scalar_type());
    TORCH_CHECK(a.numel == kAny || t.numel() == a.numel, op, ": ", a.name,
                " has ", t.numel(), " elements, expected ", a.numel);
  }
  return dtype_flag(first);
}

// A row count or width as the `int` a launcher takes.
int as_int(const char* op, const char* name, int64_t v) {
  TORCH_CHECK(v >= 0 && v <= INT_MAX, op, ": ", name, " = ", v,
              " does not fit the launcher's int");
  return (int)v;
}

// Row width N (> 0) and row count M of a LayerNorm input.
void ln_rows(const char* op, const at::Tensor& x, int* M, int* N) {
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0, op,
              ": x must have a non-empty last dim, got ", x.sizes());
  *N = as_int(op, "N", x.size(-1));
  *M = as_int(op, "M", x.numel() / *N);
}

// ---- layernorm ------------------------------------------------------------
std::vector<at::Tensor> layernorm_fwd(at::Tensor x, at::Tensor w, at::Tensor b,
                                      double eps,
                                      c10::optional<at::Tensor> res) {
  const char* op = "layernorm_fwd";
  int M, N;
  ln_rows(op, x, &M, &N);
  const int flag = check_call(op, {{"x", x, {}, kAny}, {"w", w, {}, N},
                                   {"b", b, {}, N},
                                   {"res", res, {}, x.numel()}});
  auto y = at::empty_like(x);
  auto f32 = x.options().dtype(at::kFloat);
  auto mean = at::empty({M}, f32);
  auto rstd = at::empty({M}, f32);
  at::Tensor h;
  void* res_p = nullptr;
  void* h_p = nullptr;
  if (res.has_value()) {
    h = at::empty_like(x);
    res_p = res->data_ptr();
    h_p = h.data_ptr();
  }
  check_hip(tdsa_ln_fwd(x.data_ptr(), res_p, h_p, w.data_ptr(), b.data_ptr(),
                        y.data_ptr(), mean.data_ptr<float>(),
                        rstd.data_ptr<float>(), M, N, (float)eps, flag,
                        cur_stream()),
            op);
  // mean/rstd viewed to the row shape of x
  auto row_sizes = x.sizes().vec();
  row_sizes.pop_back();
  if (res.has_value())
    return {y, mean.view(row_sizes), rstd.view(row_sizes), h};
  return {y, mean.view(row_sizes), rstd.view(row_sizes)};
}

std::vector<at::Tensor> layernorm_bwd_dx(at::Tensor dy, at::Tensor x,
                                         at::Tensor w, at::Tensor mean,
                                         at::Tensor rstd,
                                         c10::optional<at::Tensor> dh) {
  const char* op = "layernorm_bwd_dx";
  int M, N;
  ln_rows(op, x, &M, &N);
  const int flag = check_call(op, {{"x", x, {}, kAny},
                                   {"dy", dy, {}, x.numel()},
                                   {"w", w, {}, N},
                                   {"mean", mean, at::kFloat, M, true},
                                   {"rstd", rstd, at::kFloat, M, true},
                                   {"dh", dh, {}, x.numel(), true}});
  const int G = tdsa_ln_bwd_dx_stripes(M, N, flag);
  auto dx = at::empty_like(x);
  auto f32 = x.options().dtype(at::kFloat);
  auto pdw = at::empty({G, N}, f32);
  auto pdb = at::empty({G, N}, f32);
  auto meanc = mean.contiguous();
  auto rstdc = rstd.contiguous();
  at::Tensor dhc;
  void* dh_p = nullptr;
  if (dh.has_value()) {
    dhc = dh->contiguous();
    dh_p = dhc.data_ptr();
  }
  check_hip(tdsa_ln_bwd_dx(dy.data_ptr(), dh_p, x.data_ptr(), w.data_ptr(),
                           meanc.data_ptr<float>(), rstdc.data_ptr<float>(),
                           dx.data_ptr(), pdw.data_ptr<float>(),
                           pdb.data_ptr<float>(), M, N, flag, cur_stream()),
            op);
  return {dx, pdw, pdb};
}

// dtype: output dtype of dw/db (float32 or bfloat16, rounded in-kernel from
// the fp32 sums); fp32 when absent.
std::vector<at::Tensor> layernorm_bwd_dwdb(
    at::Tensor pdw, at::Tensor pdb, c10::optional<at::ScalarType> dtype) {
  const char* op = "layernorm_bwd_dwdb";
  check_call(op, {{"pdw", pdw, at::kFloat, kAny},
                  {"pdb", pdb, at::kFloat, pdw.numel()}});
  TORCH_CHECK(pdw.dim() == 2, op, ": pdw must be 2-D, got ", pdw.sizes());
  const at::ScalarType out = dtype.value_or(at::kFloat);
  TORCH_CHECK(out == at::kFloat || out == at::kBFloat16,
              "layernorm_bwd_dwdb: dtype must be float32 or bfloat16");
  const int G = as_int(op, "G", pdw.size(0));
  const int N = as_int(op, "N", pdw.size(1));
  auto dw = at::empty({N}, pdw.options().dtype(out));
  auto db = at::empty({N}, pdb.options().dtype(out));
  check_hip(tdsa_ln_bwd_dwdb(pdw.data_ptr<float>(), pdb.data_ptr<float>(),
                             dw.data_ptr(), db.data_ptr(), G, N,
                             out == at::kBFloat16, cur_stream()),
            op);
  return {dw, db};
}

// Launch geometry of the row-per-wave LayerNorm path for an (M, N) problem:
// (stripe count = backward waves, forward waves, forward batch depth,
// backward batch depth, last routed bf16 N). Waves and depths are 0 when the
// shape stays on the workgroup-per-row kernels (the stripe count never is).
std::vector<int64_t> layernorm_rowwave_geometry(int64_t M, int64_t N,
                                                bool is_bf16) {
  int fw = 0, fd = 0, bd = 0, bound = 0;
  tdsa_ln_rowwave_info((int)M, (int)N, is_bf16, &fw, &fd, &bd, &bound);
  return {tdsa_ln_bwd_dx_stripes((int)M, (int)N, is_bf16), fw, fd, bd, bound};
}

// ---- elementwise ----------------------------------------------------------
at::Tensor gelu_fwd(at::Tensor x) {
  const int flag = check_call("gelu_fwd", {{"x", x, {}, kAny}});
  auto y = at::empty_like(x);
  check_hip(tdsa_gelu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), flag,
                          cur_stream()),
            "gelu_fwd");
  return y;
}

at::Tensor gelu_bwd(at::Tensor dy, at::Tensor x) {
  const int flag = check_call("gelu_bwd", {{"x", x, {}, kAny},
                                           {"dy", dy, {}, x.numel()}});
  auto dx = at::empty_like(x);
  check_hip(tdsa_gelu_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel(),
                          flag, cur_stream()),
            "gelu_bwd");
  return dx;
}

at::Tensor column_sum(at::Tensor dy) {
  const char* op = "column_sum";
  const int flag = check_call(op, {{"dy", dy, {}, kAny}});
  TORCH_CHECK(dy.dim() == 2, "column_sum expects 2-D input");
  const int M = as_int(op, "M", dy.size(0));
  const int N = as_int(op, "N", dy.size(1));
  auto out32 = at::zeros({N}, dy.options().dtype(at::kFloat));
  auto out = at::empty({N}, dy.options());
  check_hip(tdsa_column_sum(dy.data_ptr(), out32.data_ptr<float>(),
                            out.data_ptr(), M, N, flag, cur_stream()),
            op);
  return out;
}

// ---- embedding ------------------------------------------------------------
at::Tensor embedding_fwd(at::Tensor weight, at::Tensor idx) {
  const char* op = "embedding_fwd";
  const int flag = check_call(op, {{"weight", weight, {}, kAny},
                                   {"idx", idx, at::kLong, kAny}});
  TORCH_CHECK(weight.dim() == 2, op, ": weight must be 2-D, got ",
              weight.sizes());
  const long long R = idx.numel();
  const int D = as_int(op, "D", weight.size(1));
  auto out = at::empty({R, (long long)D}, weight.options());
  check_hip(tdsa_embedding_fwd(weight.data_ptr(), (const long long*)idx.data_ptr<int64_t>(),
                               out.data_ptr(), R, D, flag, cur_stream()),
            op);
  return out;
}

at::Tensor embedding_bwd(at::Tensor dy, at::Tensor idx, int64_t num_embeddings,
                         int64_t padding_idx) {
  const char* op = "embedding_bwd";
  const int flag = check_call(op, {{"dy", dy, {}, kAny},
                                   {"idx", idx, at::kLong, kAny}});
  const long long R = idx.numel();
  TORCH_CHECK(dy.dim() >= 1 && dy.numel() == R * dy.size(-1), op,
              ": dy must have idx.numel() = ", R, " rows, got ", dy.sizes());
  const int D = as_int(op, "D", dy.size(-1));
  auto dw32 = at::zeros({num_embeddings, (long long)D},
                        dy.options().dtype(at::kFloat));
  // stable sort: equal indices keep their dy-row order, so every table row
  // is summed in one fixed order
  auto sorted = at::sort(idx.reshape({-1}), /*stable=*/true, /*dim=*/0,
                         /*descending=*/false);
  auto sidx = std::get<0>(sorted).contiguous();
  auto perm = std::get<1>(sorted).contiguous();
  // scratch for the piece sums of indices that occur more than 32 times
  auto part = at::empty({R, (long long)D}, dy.options().dtype(at::kFloat));
  check_hip(tdsa_embedding_bwd(dy.data_ptr(), (const long long*)sidx.data_ptr<int64_t>(),
                               (const long long*)perm.data_ptr<int64_t>(),
                               dw32.data_ptr<float>(), part.data_ptr<float>(),
                               R, D, padding_idx, flag, cur_stream()),
            op);
  return dw32;
}

// ---- cross entropy --------------------------------------------------------
std::vector<at::Tensor> cross_entropy_fwd(at::Tensor logits, at::Tensor targets,
                                          int64_t ignore_index) {
  const char* op = "cross_entropy_fwd";
  TORCH_CHECK(logits.dim() == 2, op, ": logits must be 2-D");
  const long long R = logits.size(0);
  const int V = as_int(op, "V", logits.size(1));
  const int flag = check_call(op, {{"logits", logits, {}, kAny},
                                   {"targets", targets, at::kLong, R}});
  auto f32 = logits.options().dtype(at::kFloat);
  auto lse = at::empty({R}, f32);
  // per-row losses, summed below in torch's fixed reduction order
  auto row_loss = at::empty({R}, f32);
  auto n_valid32 = at::zeros({}, logits.options().dtype(at::kInt));
  check_hip(tdsa_ce_fwd(logits.data_ptr(), (const long long*)targets.data_ptr<int64_t>(),
                        lse.data_ptr<float>(), row_loss.data_ptr<float>(),
                        n_valid32.data_ptr<int>(), R, V, ignore_index, flag,
                        cur_stream()),
            op);
  return {row_loss.sum(), lse, n_valid32.to(at::kLong)};
}

at::Tensor cross_entropy_bwd(at::Tensor logits, at::Tensor targets,
                             at::Tensor lse, double dloss, int64_t n_valid,
                             int64_t ignore_index,
                             c10::optional<at::Tensor> out) {
  const char* op = "cross_entropy_bwd";
  TORCH_CHECK(logits.dim() == 2, op, ": logits must be 2-D");
  const long long R = logits.size(0);
  const int V = as_int(op, "V", logits.size(1));
  // out: e.g. a row-slice of the fused-CE dlogits buffer
  at::Tensor dlogits = out.has_value() ? *out : at::empty_like(logits);
  const int flag = check_call(op, {{"logits", logits, {}, kAny},
                                   {"targets", targets, at::kLong, R},
                                   {"lse", lse, at::kFloat, R},
                                   {"out", dlogits, {}, kAny}});
  TORCH_CHECK(dlogits.sizes() == logits.sizes(), op,
              ": out must have logits' sizes ", logits.sizes(), ", got ",
              dlogits.sizes());
  const float scale = (float)(dloss / (double)std::max<int64_t>(n_valid, 1));
  check_hip(tdsa_ce_bwd(logits.data_ptr(), (const long long*)targets.data_ptr<int64_t>(),
                        lse.data_ptr<float>(), dlogits.data_ptr(), R, V, scale,
                        ignore_index, flag, cur_stream()),
            op);
  return dlogits;
}

// ---- fused optimizers -----------------------------------------------------
// Data pointer of tensor `name` of entry i, after the checks every tensor of
// a multi-tensor launch must pass. State tensors (`state`) are fp32.
void* entry_ptr(const char* what, size_t i, const char* name,
                const at::Tensor& t, int64_t numel, bool state) {
  TORCH_CHECK(t.is_cuda(), what, ": ", name, "[", i, "] must be on GPU");
  TORCH_CHECK(t.is_contiguous(), what, ": ", name, "[", i,
              "] must be contiguous");
  const auto st = t.scalar_type();
  TORCH_CHECK(st == at::kFloat || (!state && st == at::kBFloat16), what, ": ",
              name, "[", i, "] must be float32",
              state ? "" : " or bfloat16", ", got ", st);
  TORCH_CHECK(t.numel() == numel, what, ": ", name, "[", i, "] has ",
              t.numel(), " elements, param[", i, "] has ", numel);
  return t.data_ptr();
}

float* state_ptr(const char* what, size_t i, const char* name,
                 const c10::optional<at::Tensor>& t, int64_t numel) {
  if (!t.has_value()) return nullptr;
  return (float*)entry_ptr(what, i, name, *t, numel, true);
}

// The fields every descriptor starts from: param, grad, numel, dtype flags.
template <typename Desc>
void fill_param_grad(Desc& d, const char* what, size_t i, const at::Tensor& p,
                     const at::Tensor& g) {
  d.numel = p.numel();
  d.p = entry_ptr(what, i, "param", p, d.numel, false);
  d.g = entry_ptr(what, i, "grad", g, d.numel, false);
  d.param_bf16 = dtype_flag(p);
  d.grad_bf16 = dtype_flag(g);
}

// Builds the chunk table for `descs`, ships [descs][chunks] as one small
// device blob and calls launch(blob, ndescs, nchunks).
template <typename Desc, typename Launch>
void launch_optim_multi(const char* what, const std::vector<Desc>& descs,
                        const at::Device& device, Launch launch) {
  std::vector<tdsa::ChunkRef> chunks;
  chunks.reserve(1024);
  for (size_t i = 0; i < descs.size(); ++i) {
    const long long nch = (descs[i].numel + tdsa::kOptimChunkElems - 1) /
                          tdsa::kOptimChunkElems;
    for (long long c = 0; c < nch; ++c) chunks.push_back({(int)i, (int)c});
  }
  const size_t desc_bytes = descs.size() * sizeof(Desc);
  const size_t chunk_bytes = chunks.size() * sizeof(tdsa::ChunkRef);
  auto host = at::empty({(long long)(desc_bytes + chunk_bytes)},
                        at::TensorOptions().dtype(at::kByte));
  std::memcpy(host.data_ptr(), descs.data(), desc_bytes);
  std::memcpy((char*)host.data_ptr() + desc_bytes, chunks.data(), chunk_bytes);
  auto dev = host.to(device);
  check_hip(launch(dev.data_ptr(), (int)descs.size(), (int)chunks.size()),
            what);
}

// The optional gradient scale of an update launch: one fp32 number on the
// parameters' device, read by the kernel (no host copy). nullptr when absent.
const float* grad_scale_ptr(const char* what,
                            const c10::optional<at::Tensor>& grad_scale,
                            const at::Device& device) {
  if (!grad_scale.has_value()) return nullptr;
  const at::Tensor& s = *grad_scale;
  TORCH_CHECK(s.scalar_type() == at::kFloat, what,
              ": grad_scale must be float32, got ", s.scalar_type());
  TORCH_CHECK(s.numel() == 1, what, ": grad_scale has ", s.numel(),
              " elements, expected 1");
  TORCH_CHECK(s.device() == device, what, ": grad_scale is on ", s.device(),
              ", the parameters on ", device);
  return s.data_ptr<float>();
}

// One fused launch for a whole parameter list. vmaxs: all present (amsgrad)
// or all absent.
void adamw_step_multi(std::vector<at::Tensor> params,
                      std::vector<at::Tensor> grads,
                      std::vector<at::Tensor> ms, std::vector<at::Tensor> vs,
                      std::vector<c10::optional<at::Tensor>> masters,
                      std::vector<c10::optional<at::Tensor>> vmaxs,
                      double lr, double b1, double b2, double eps, double wd,
                      int64_t step, c10::optional<at::Tensor> grad_scale) {
  const char* what = "adamw_step_multi";
  const size_t n = params.size();
  TORCH_CHECK(grads.size() == n && ms.size() == n && vs.size() == n &&
              masters.size() == n && vmaxs.size() == n,
              what, ": length mismatch");
  if (n == 0) return;
  const float* gscale = grad_scale_ptr(what, grad_scale, params[0].device());
  const bool amsgrad = vmaxs[0].has_value();
  std::vector<tdsa::AdamTensorDesc> descs(n);
  for (size_t i = 0; i < n; ++i) {
    auto& d = descs[i];
    fill_param_grad(d, what, i, params[i], grads[i]);
    d.m = state_ptr(what, i, "m", ms[i], d.numel);
    d.v = state_ptr(what, i, "v", vs[i], d.numel);
    d.master = state_ptr(what, i, "master", masters[i], d.numel);
    d.vmax = state_ptr(what, i, "vmax", vmaxs[i], d.numel);
    TORCH_CHECK((d.vmax != nullptr) == amsgrad, what, ": vmax[", i,
                "] must be given for every entry or for none");
  }
  launch_optim_multi(what, descs, params[0].device(),
                     [&](const void* blob, int ndescs, int nchunks) {
    return tdsa_adamw_multi(blob, ndescs, nchunks, amsgrad, (float)lr,
                            (float)b1, (float)b2, (float)eps, (float)wd, step,
                            gscale, cur_stream());
  });
}

// first[i]: entry i takes its first step (its buf is set to the gradient).
void sgd_step_multi(std::vector<at::Tensor> params,
                    std::vector<at::Tensor> grads,
                    std::vector<c10::optional<at::Tensor>> bufs,
                    std::vector<c10::optional<at::Tensor>> masters,
                    std::vector<bool> first, double lr, double momentum,
                    double dampening, double wd, bool nesterov,
                    bool maximize, c10::optional<at::Tensor> grad_scale) {
  const char* what = "sgd_step_multi";
  const size_t n = params.size();
  TORCH_CHECK(grads.size() == n && bufs.size() == n && masters.size() == n &&
              first.size() == n, what, ": length mismatch");
  if (n == 0) return;
  const float* gscale = grad_scale_ptr(what, grad_scale, params[0].device());
  std::vector<tdsa::SgdTensorDesc> descs(n);
  for (size_t i = 0; i < n; ++i) {
    auto& d = descs[i];
    fill_param_grad(d, what, i, params[i], grads[i]);
    d.buf = state_ptr(what, i, "buf", bufs[i], d.numel);
    d.master = state_ptr(what, i, "master", masters[i], d.numel);
    d.first = first[i];
  }
  launch_optim_multi(what, descs, params[0].device(),
                     [&](const void* blob, int ndescs, int nchunks) {
    return tdsa_sgd_multi(blob, ndescs, nchunks, (float)lr, (float)momentum,
                          (float)dampening, (float)wd, nesterov, maximize,
                          gscale, cur_stream());
  });
}

// fp32 sum of squares of every gradient (bf16 and fp32 mixed) as a 0-dim
// tensor on their device: the second user of the optimizer launch's blob.
at::Tensor grad_sumsq_multi(std::vector<at::Tensor> grads) {
  const char* what = "grad_sumsq_multi";
  const size_t n = grads.size();
  TORCH_CHECK(n > 0, what, ": empty gradient list");
  std::vector<tdsa::GradNormDesc> descs(n);
  long long nchunks = 0;
  for (size_t i = 0; i < n; ++i) {
    auto& d = descs[i];
    TORCH_CHECK(grads[i].device() == grads[0].device(), what, ": grad[", i,
                "] is on ", grads[i].device(), ", grad[0] on ",
                grads[0].device());
    d.numel = grads[i].numel();
    d.g = entry_ptr(what, i, "grad", grads[i], d.numel, false);
    d.bf16 = dtype_flag(grads[i]);
    nchunks += (d.numel + tdsa::kOptimChunkElems - 1) / tdsa::kOptimChunkElems;
  }
  auto f32 = grads[0].options().dtype(at::kFloat);
  auto partials = at::empty({nchunks}, f32);
  auto out = at::empty({}, f32);
  launch_optim_multi(what, descs, grads[0].device(),
                     [&](const void* blob, int ndescs, int nch) {
    return tdsa_grad_sumsq_multi(blob, ndescs, nch,
                                 partials.data_ptr<float>(),
                                 out.data_ptr<float>(), cur_stream());
  });
  return out;
}

// ---- TN GEMM (linear dW autotuner candidate) ------------------------------
at::Tensor gemm_tn(at::Tensor dy2, at::Tensor x2) {
  const char* op = "gemm_tn";
  check_call(op, {{"dy2", dy2, at::kBFloat16, kAny},
                  {"x2", x2, at::kBFloat16, kAny}});
  TORCH_CHECK(dy2.dim() == 2 && x2.dim() == 2, "gemm_tn expects 2-D inputs");
  TORCH_CHECK(dy2.size(0) == x2.size(0), "gemm_tn: reduction dims differ");
  const long long M = dy2.size(0);
  const int N = as_int(op, "N", dy2.size(1));
  const int K = as_int(op, "K", x2.size(1));
  const int splits = tdsa_gemm_tn_splits(M, N, K);
  TORCH_CHECK(splits > 0, "gemm_tn: unsupported shape (need M%64==0, "
              "N%128==0, K%128==0), got ", M, "x", N, "/", K);
  auto f32 = dy2.options().dtype(at::kFloat);
  // one [N, K] slab per M-split, summed here in slab order (deterministic)
  auto dw32 = at::empty({(long long)splits, (long long)N, (long long)K}, f32);
  check_hip(tdsa_gemm_tn(dy2.data_ptr(), x2.data_ptr(),
                         dw32.data_ptr<float>(), M, N, K, cur_stream()),
            "gemm_tn");
  return (splits > 1 ? dw32.sum(0) : dw32.select(0, 0)).to(at::kBFloat16);
}

// ---- transpose / linear dX in the forward's GEMM layout -------------------
// out[K, N] = w[N, K]^T, bit for bit.
at::Tensor transpose_bf16(at::Tensor w) {
  const char* op = "transpose_bf16";
  check_call(op, {{"w", w, at::kBFloat16, kAny}});
  TORCH_CHECK(w.dim() == 2, op, ": w must be 2-D, got ", w.sizes());
  const long long N = w.size(0), K = w.size(1);
  TORCH_CHECK(N > 0 && K > 0 && N % 64 == 0 && K % 64 == 0, op,
              ": both dims must be positive multiples of 64, got ", w.sizes());
  auto out = at::empty({K, N}, w.options());
  check_hip(tdsa_transpose_bf16(w.data_ptr(), out.data_ptr(), N, K,
                                cur_stream()),
            op);
  return out;
}

// dx[M, K] = dy2[M, N] @ w[N, K] as the library's forward-layout GEMM: w is
// transposed on the fly (never kept: the weight may change between calls) and
// the product goes through at::linear, so TunableOp and its cache apply.
at::Tensor linear_dx_nt(at::Tensor dy2, at::Tensor w) {
  const char* op = "linear_dx_nt";
  check_call(op, {{"dy2", dy2, at::kBFloat16, kAny},
                  {"w", w, at::kBFloat16, kAny}});
  TORCH_CHECK(dy2.dim() == 2 && w.dim() == 2, op, " expects 2-D inputs, got ",
              dy2.sizes(), " and ", w.sizes());
  TORCH_CHECK(dy2.size(1) == w.size(0), op, ": dy2 ", dy2.sizes(),
              " does not contract with w ", w.sizes());
  return at::linear(dy2, transpose_bf16(w));
}

// ---- attention ------------------------------------------------------------
// One pass over an attention call's bf16 tensors, q first. The kernels use
// q's extents and, per group, one tensor's strides (`lead`: q for q/k/v, o for
// o/dout, dq for dq/dk/dv), so any other shape or stride stops here.
struct AttnTensor { const char* name; const at::Tensor &t, &lead; };
static void check_attn_call(std::initializer_list<AttnTensor> tensors,
                            double dropout_p) {
  const at::Tensor& q = tensors.begin()->t;
  for (const auto& [name, t, lead] : tensors) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.dim() == 4 && t.size(3) == 64, name,
                ": attention kernel requires (B,H,T,64)");
    TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16");
    TORCH_CHECK(t.stride(3) == 1, name, " last dim must be contiguous");
    TORCH_CHECK(t.sizes() == q.sizes(), name, " must have q's sizes ",
                q.sizes(), ", got ", t.sizes());
    TORCH_CHECK(t.strides() == lead.strides(), name,
                ": q/k/v, o/dout and dq/dk/dv must each share strides");
  }
  TORCH_CHECK(q.size(2) % 64 == 0, "attention kernel requires T % 64 == 0");
  TORCH_CHECK(dropout_p >= 0.0 && dropout_p < 1.0, "bad dropout_p");
}

static std::array<long long, 3> strides3(const at::Tensor& t) {
  return {t.stride(0), t.stride(1), t.stride(2)};
}

std::vector<at::Tensor> attention_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                      double scale,
                                      c10::optional<at::Tensor> out,
                                      double dropout_p, int64_t seed) {
  at::Tensor o = out.has_value() ? *out : at::empty_like(q);
  check_attn_call({{"q", q, q}, {"k", k, q}, {"v", v, q}, {"out", o, o}},
                  dropout_p);
  const long long B = q.size(0), H = q.size(1), T = q.size(2);
  auto lse = at::empty({B, H, T}, q.options().dtype(at::kFloat));
  check_hip(tdsa_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                          o.data_ptr(), lse.data_ptr<float>(), B, H, (int)T,
                          (float)scale, strides3(q).data(), strides3(o).data(),
                          (float)dropout_p, (unsigned long long)seed,
                          cur_stream()),
            "attention_fwd");
  return {o, lse};
}

std::vector<at::Tensor> attention_bwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                      at::Tensor o, at::Tensor lse,
                                      at::Tensor dout, double scale,
                                      c10::optional<at::Tensor> dq_out,
                                      c10::optional<at::Tensor> dk_out,
                                      c10::optional<at::Tensor> dv_out,
                                      double dropout_p, int64_t seed) {
  at::Tensor dq = dq_out.has_value() ? *dq_out : at::empty_like(q);
  at::Tensor dk = dk_out.has_value() ? *dk_out : at::empty_like(k);
  at::Tensor dv = dv_out.has_value() ? *dv_out : at::empty_like(v);
  check_attn_call({{"q", q, q}, {"k", k, q}, {"v", v, q}, {"o", o, o},
                   {"dout", dout, o}, {"dq", dq, dq}, {"dk", dk, dq},
                   {"dv", dv, dq}}, dropout_p);
  const long long B = q.size(0), H = q.size(1), T = q.size(2);
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat &&
                  lse.numel() == B * H * T,
              "lse must be fp32 on GPU with B*H*T elements, got ", lse.sizes());
  auto lsec = lse.contiguous();
  auto delta = at::empty({B * H * T}, q.options().dtype(at::kFloat));
  check_hip(tdsa_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                          o.data_ptr(), lsec.data_ptr<float>(), dout.data_ptr(),
                          dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                          delta.data_ptr<float>(), B, H, (int)T, (float)scale,
                          strides3(q).data(), strides3(o).data(),
                          strides3(dq).data(), (float)dropout_p,
                          (unsigned long long)seed, cur_stream()),
            "attention_bwd");
  return {dq, dk, dv};
}

// ---- debug probes ---------------------------------------------------------
at::Tensor dbg_mfma(at::Tensor A, at::Tensor B, int64_t variant) {
  check_call("dbg_mfma", {{"A", A, at::kBFloat16, 16 * 32},
                          {"B", B, at::kBFloat16, 32 * 16}});
  auto D = at::zeros({16, 16}, A.options().dtype(at::kFloat));
  check_hip(tdsa_dbg_mfma(A.data_ptr(), B.data_ptr(), D.data_ptr<float>(),
                          (int)variant, cur_stream()),
            "dbg_mfma");
  return D;
}

at::Tensor dbg_mfma32(at::Tensor A, at::Tensor B) {
  check_call("dbg_mfma32", {{"A", A, at::kBFloat16, 32 * 16},
                            {"B", B, at::kBFloat16, 16 * 32}});
  auto D = at::zeros({32, 32}, A.options().dtype(at::kFloat));
  check_hip(tdsa_dbg_mfma32(A.data_ptr(), B.data_ptr(), D.data_ptr<float>(),
                            cur_stream()),
            "dbg_mfma32");
  return D;
}

at::Tensor dbg_stage(at::Tensor in, int64_t transposed) {
  check_call("dbg_stage", {{"in", in, at::kBFloat16, 64 * 64}});
  auto out = at::zeros_like(in);
  check_hip(tdsa_dbg_stage(in.data_ptr(), out.data_ptr(), (int)transposed,
                           cur_stream()),
            "dbg_stage");
  return out;
}

at::Tensor dbg_tr16(at::Tensor in) {
  check_call("dbg_tr16", {{"in", in, at::kBFloat16, 64 * 64}});
  auto out = at::zeros({2, 4, 2, 4, 64}, in.options().dtype(at::kFloat));
  check_hip(tdsa_dbg_tr16(in.data_ptr(), out.data_ptr<float>(), cur_stream()),
            "dbg_tr16");
  return out;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("dbg_mfma", &dbg_mfma);
  mod.def("dbg_mfma32", &dbg_mfma32);
  mod.def("dbg_stage", &dbg_stage);
  mod.def("dbg_tr16", &dbg_tr16);
  mod.def("layernorm_fwd", &layernorm_fwd, py::arg("x"), py::arg("w"),
          py::arg("b"), py::arg("eps"), py::arg("res") = py::none());
  mod.def("layernorm_bwd_dx", &layernorm_bwd_dx, py::arg("dy"), py::arg("x"),
          py::arg("w"), py::arg("mean"), py::arg("rstd"),
          py::arg("dh") = py::none());
  mod.def("layernorm_bwd_dwdb", &layernorm_bwd_dwdb, py::arg("pdw"),
          py::arg("pdb"), py::arg("dtype") = py::none());
  mod.def("layernorm_rowwave_geometry", &layernorm_rowwave_geometry,
          py::arg("M"), py::arg("N"), py::arg("is_bf16") = true);
  mod.def("gelu_fwd", &gelu_fwd);
  mod.def("gelu_bwd", &gelu_bwd);
  mod.def("column_sum", &column_sum);
  mod.def("embedding_fwd", &embedding_fwd);
  mod.def("embedding_bwd", &embedding_bwd);
  mod.def("cross_entropy_fwd", &cross_entropy_fwd);
  mod.def("cross_entropy_bwd", &cross_entropy_bwd, py::arg("logits"),
          py::arg("targets"), py::arg("lse"), py::arg("dloss"),
          py::arg("n_valid"), py::arg("ignore_index"),
          py::arg("out") = py::none());
  mod.def("gemm_tn", &gemm_tn);
  mod.def("transpose_bf16", &transpose_bf16);
  mod.def("linear_dx_nt", &linear_dx_nt);
  mod.def("adamw_step_multi", &adamw_step_multi, py::arg("params"),
          py::arg("grads"), py::arg("ms"), py::arg("vs"), py::arg("masters"),
          py::arg("vmaxs"), py::arg("lr"), py::arg("b1"), py::arg("b2"),
          py::arg("eps"), py::arg("wd"), py::arg("step"),
          py::arg("grad_scale") = py::none());
  mod.def("sgd_step_multi", &sgd_step_multi, py::arg("params"),
          py::arg("grads"), py::arg("bufs"), py::arg("masters"),
          py::arg("first"), py::arg("lr"), py::arg("momentum"),
          py::arg("dampening"), py::arg("wd"), py::arg("nesterov"),
          py::arg("maximize"), py::arg("grad_scale") = py::none());
  mod.def("grad_sumsq_multi", &grad_sumsq_multi, py::arg("grads"));
  mod.def("attention_fwd", &attention_fwd, py::arg("q"), py::arg("k"),
          py::arg("v"), py::arg("scale"), py::arg("out") = py::none(),
          py::arg("dropout_p") = 0.0, py::arg("seed") = 0);
  mod.def("attention_bwd", &attention_bwd, py::arg("q"), py::arg("k"),
          py::arg("v"), py::arg("o"), py::arg("lse"), py::arg("dout"),
          py::arg("scale"), py::arg("dq") = py::none(),
          py::arg("dk") = py::none(), py::arg("dv") = py::none(),
          py::arg("dropout_p") = 0.0, py::arg("seed") = 0);
}
