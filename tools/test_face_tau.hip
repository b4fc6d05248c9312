// tools/test_face_tau.hip -- glsmath::face_tau_t (the series) and glsmath::face_tau_tab_t (the tables, from LDS as the cube-node
// kernel calls it) over a grid the caller supplies; tests/test_gpu_face_tau.py compares both with numpy's pow.
//   test_face_tau in.bin out.bin     in: int64 n, then n x (u, eta) doubles;  out: n x (series(u), tab(u), series_sq(u^2), tab_sq(u^2))
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "gls_device_math.hpp"

using namespace nin::glsmath;

__global__ __launch_bounds__(256) void k_tau(const double *in, int64_t n, double *out) {
    __shared__ double tab[TAU_TAB_DOUBLES];
    tau_table_to_lds(tab);
    __syncthreads();
    const lds_cdouble_ptr t = (lds_cdouble_ptr)tab;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double u = in[2 * i], eta = in[2 * i + 1];
        out[4 * i + 0] = face_tau_t<false>(u, eta);
        out[4 * i + 1] = face_tau_tab_t<false>(u, eta, t);
        out[4 * i + 2] = face_tau_t<true>(u * u, eta);
        out[4 * i + 3] = face_tau_tab_t<true>(u * u, eta, t);
    }
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: test_face_tau in.bin out.bin\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    int64_t n = 0;
    if (!f || fread(&n, sizeof n, 1, f) != 1 || n <= 0 || n > (1 << 24)) { fprintf(stderr, "bad input\n"); return 1; }
    std::vector<double> in(2 * (size_t)n), out(4 * (size_t)n);
    if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) { fprintf(stderr, "short input\n"); return 1; }
    fclose(f);
    double *din = nullptr, *dout = nullptr;
    CHECK(hipMalloc(&din, in.size() * sizeof(double)));
    CHECK(hipMalloc(&dout, out.size() * sizeof(double)));
    CHECK(hipMemcpy(din, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_tau, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, din, n, dout);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), dout, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { fprintf(stderr, "cannot write\n"); return 1; }
    fclose(f);
    printf("all ok: %lld points\n", (long long)n);
    return 0;
}
