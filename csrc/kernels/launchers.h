// Every extern "C" launcher of the kernel files, declared once.
//
// bind.cpp calls through these prototypes and each .hip file that defines a
// launcher includes them too, so a definition whose argument list drifts is
// a compile error in that file ("conflicting types") instead of a call that
// links and hands a kernel the wrong arguments. Plain C types and the HIP
// runtime API only: the host compiler reads this header as well.
//
// Common to all: tensor arguments are device pointers to contiguous data
// unless strides are passed; is_bf16 picks bf16 (1) or fp32 (0) for the
// `void*` tensors; the launch goes to `stream`; the return value is the
// launch status, hipErrorInvalidValue for a shape the kernels do not take.
#pragma once

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

// ---- layernorm.hip ----------------------------------------------------------
// x, y [M, N]; w, b [N]; mean, rstd fp32 [M]. res/h: optional fused residual
// (h = x + res is written and normalised); both null for the plain form.
// N must be a whole number of 16-byte vectors.
hipError_t tdsa_ln_fwd(const void* x, const void* res, void* h, const void* w,
                       const void* b, void* y, float* mean, float* rstd,
                       int M, int N, float eps, int is_bf16,
                       hipStream_t stream);
// Stripe count G the backward will use: the caller sizes pdw/pdb as [G, N].
int tdsa_ln_bwd_dx_stripes(int M, int N, int is_bf16);
// Row-per-wave geometry for tests and tools: forward waves and batch depths
// (0 when the shape is not routed there) and the last routed bf16 N.
void tdsa_ln_rowwave_info(int M, int N, int is_bf16, int* fwd_waves,
                          int* fwd_depth, int* bwd_depth, int* bound);
// dh: optional residual-stream gradient added into dx (null for none).
// pdw, pdb fp32 [G, N] receive the stripe partials (need not be initialised).
hipError_t tdsa_ln_bwd_dx(const void* dy, const void* dh, const void* x,
                          const void* w, const float* mean, const float* rstd,
                          void* dx, float* pdw, float* pdb, int M, int N,
                          int is_bf16, hipStream_t stream);
// dw, db [N] = column sums of pdw, pdb [G, N]; out_bf16 picks their dtype.
hipError_t tdsa_ln_bwd_dwdb(const float* pdw, const float* pdb, void* dw,
                            void* db, int G, int N, int out_bf16,
                            hipStream_t stream);

// ---- elementwise.hip --------------------------------------------------------
// y[n] = gelu(x[n]), any n.
hipError_t tdsa_gelu_fwd(const void* x, void* y, long long n, int is_bf16,
                         hipStream_t stream);
// dx[n] = dy[n] * gelu'(x[n]), any n.
hipError_t tdsa_gelu_bwd(const void* dy, const void* x, void* dx, long long n,
                         int is_bf16, hipStream_t stream);
// out[N] = column sums of dy [M, N]. out32 fp32 [N] must be zero-filled; out
// (dy's dtype) receives the cast.
hipError_t tdsa_column_sum(const void* dy, float* out32, void* out, int M,
                           int N, int is_bf16, hipStream_t stream);

// ---- embedding.hip ----------------------------------------------------------
// out [R, D] = weight[idx[r]]; every idx must be a valid row of weight.
hipError_t tdsa_embedding_fwd(const void* weight, const long long* idx,
                              void* out, long long R, int D, int is_bf16,
                              hipStream_t stream);
// idx [R] sorted ascending, perm [R] the dy row of each sorted entry. dw32
// fp32 [V, D] must be zero-filled; part fp32 [R, D] is scratch (need not be
// initialised). padding_idx: the row to skip, -1 for none.
hipError_t tdsa_embedding_bwd(const void* dy, const long long* idx,
                              const long long* perm, float* dw32, float* part,
                              long long R, int D, long long padding_idx,
                              int is_bf16, hipStream_t stream);

// ---- cross_entropy.hip ------------------------------------------------------
// logits [R, V] with V a whole number of 16-byte vectors; targets [R] in
// [0, V) or ignore_index. Writes lse, row_loss fp32 [R] (0 for ignored rows)
// and adds the count of valid rows to n_valid, which must be zero-filled.
hipError_t tdsa_ce_fwd(const void* logits, const long long* targets,
                       float* lse, float* row_loss, int* n_valid, long long R,
                       int V, long long ignore_index, int is_bf16,
                       hipStream_t stream);
// dlogits [R, V] = (softmax - onehot) * scale, 0 for ignored rows; lse from
// the forward. Same V precondition.
hipError_t tdsa_ce_bwd(const void* logits, const long long* targets,
                       const float* lse, void* dlogits, long long R, int V,
                       float scale, long long ignore_index, int is_bf16,
                       hipStream_t stream);

// ---- optim.hip --------------------------------------------------------------
// blob: ndescs tensor descriptors followed by nchunks ChunkRef entries
// (optim_desc.h), on the device. amsgrad: every descriptor carries a vmax.
// step: the global 1-based optimizer step. gscale: one fp32 number on the
// device that every gradient element is multiplied by before the update
// (the clip coefficient); nullptr: the gradients are used as they are.
hipError_t tdsa_adamw_multi(const void* blob, int ndescs, int nchunks,
                            int amsgrad, float lr, float b1, float b2,
                            float eps, float wd, long long step,
                            const float* gscale, hipStream_t stream);
hipError_t tdsa_sgd_multi(const void* blob, int ndescs, int nchunks, float lr,
                          float momentum, float dampening, float wd,
                          int nesterov, int maximize, const float* gscale,
                          hipStream_t stream);

// ---- gradnorm.hip -----------------------------------------------------------
// Sum of squares of every gradient of the blob ([GradNormDesc][ChunkRef]) as
// one fp32 number at `out`. partials: nchunks floats of scratch. nchunks may
// be 0 (every tensor empty): out = 0.
hipError_t tdsa_grad_sumsq_multi(const void* blob, int ndescs, int nchunks,
                                 float* partials, float* out,
                                 hipStream_t stream);

// ---- attention.hip ----------------------------------------------------------
// bf16 (B, H, T, 64) tensors with T % 64 == 0 and a contiguous last dim.
// sq, so, sd: {b, h, t} strides in elements of q/k/v, of o/dout and of
// dq/dk/dv. lse fp32 [B, H, T] contiguous. dropout_p > 0 applies the mask
// that `seed` generates, the same in forward and backward.
hipError_t tdsa_attn_fwd(const void* q, const void* k, const void* v, void* o,
                         float* lse, long long B, long long H, int T,
                         float scale, const long long* sq, const long long* so,
                         float dropout_p, unsigned long long seed,
                         hipStream_t stream);
// delta fp32 [B*H*T] is scratch (need not be initialised).
hipError_t tdsa_attn_bwd(const void* q, const void* k, const void* v,
                         const void* o, const float* lse, const void* dout,
                         void* dq, void* dk, void* dv, float* delta,
                         long long B, long long H, int T, float scale,
                         const long long* sq, const long long* so,
                         const long long* sd, float dropout_p,
                         unsigned long long seed, hipStream_t stream);

// ---- gemm_tn.hip ------------------------------------------------------------
// Split count for dw = dy[M, N]^T x[M, K]; <= 0 means the shape is not taken
// (needs M % 64 == 0, N % 128 == 0, K % 128 == 0).
int tdsa_gemm_tn_splits(long long M, int N, int K);
// dy, x bf16; dw fp32 [splits, N, K], one slab per split (need not be
// initialised), summed by the caller.
hipError_t tdsa_gemm_tn(const void* dy, const void* x, float* dw, long long M,
                        int N, int K, hipStream_t stream);

// ---- transpose.hip ----------------------------------------------------------
// out bf16 [K, N] = in bf16 [N, K] transposed; N and K multiples of 64. in and
// out must not overlap.
hipError_t tdsa_transpose_bf16(const void* in, void* out, long long N,
                               long long K, hipStream_t stream);

// ---- debug.hip --------------------------------------------------------------
// Fragment-layout probes on one wave. A [16, 32], B [32, 16] bf16 -> D fp32
// [16, 16]; variant picks the A/B fragment layout.
hipError_t tdsa_dbg_mfma(const void* A, const void* B, float* D, int variant,
                         hipStream_t stream);
// A [32, 16], B [16, 32] bf16 -> D fp32 [32, 32].
hipError_t tdsa_dbg_mfma32(const void* A, const void* B, float* D,
                           hipStream_t stream);
// in, out bf16 [64, 64], through swizzled LDS, transposed or not.
hipError_t tdsa_dbg_stage(const void* in, void* out, int transposed,
                          hipStream_t stream);
// in bf16 [64, 64] -> out fp32 [2, 4, 2, 4, 64].
hipError_t tdsa_dbg_tr16(const void* in, float* out, hipStream_t stream);

#ifdef __cplusplus
}  // extern "C"
#endif
