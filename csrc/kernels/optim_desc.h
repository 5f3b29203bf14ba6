// Device-blob layout of the multi-tensor optimizer launches, shared by the
// host code that fills it (bind.cpp) and the kernels that read it
// (optim.hip, gradnorm.hip). Plain C++: no HIP or torch types.
//
// blob = [ndescs x *TensorDesc][nchunks x ChunkRef], device memory. Each
// workgroup takes one ChunkRef at a time: kOptimChunkElems elements of one
// tensor.
#pragma once

namespace tdsa {

constexpr int kOptimChunkElems = 1 << 16;

struct AdamTensorDesc {
  void* p;
  const void* g;
  float* m;
  float* v;
  float* master;  // nullptr when param is fp32
  float* vmax;    // nullptr without amsgrad
  long long numel;
  int param_bf16;
  int grad_bf16;
};

struct SgdTensorDesc {
  void* p;
  const void* g;
  float* buf;     // nullptr without momentum
  float* master;  // nullptr when param is fp32
  long long numel;
  int param_bf16;
  int grad_bf16;
  int first;      // this tensor's first step: buf is set to the gradient
};

// One gradient of the sum-of-squares launch (gradnorm.hip).
struct GradNormDesc {
  const void* g;
  long long numel;
  int bf16;
};

struct ChunkRef {
  int tensor;
  int chunk;
};

}  // namespace tdsa
