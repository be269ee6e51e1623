// TEST INFRASTRUCTURE (tests/test_gru_gates_gpu.py): the gate nonlinearities of the GRU recurrence on their own.  The
// persistent kernels compute them with fast_sigmoid / fast_tanh (gru_persist_common.h: hardware exp2 / rcp), the launch-per-step
// kernels with sigmoidf_ (ds2_common.h) / tanhf; all are __device__ inlines, so this kernel includes the headers and maps an
// array through the four of them.  Built by csrc/build.py with the library's own flags into tests/libgate_functions.so; not part
// of the library or its ABI.
#include "gru_persist_common.h"

__global__ __launch_bounds__(256) void gate_functions_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float v = x[i];
        y[i] = fast_sigmoid(v);
        y[n + i] = fast_tanh(v);
        y[2 * n + i] = sigmoidf_(v);
        y[3 * n + i] = tanhf(v);
    }
}

// x (n) -> y (4, n) = fast_sigmoid | fast_tanh | sigmoidf_ | tanhf, device pointers.  0 = launched.
extern "C" int gate_functions(const float* x, float* y, size_t n, void* stream) {
    if (!x || !y || n == 0) return -1;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(gate_functions_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, (hipStream_t)stream,
                       x, y, n);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
