// grid_update.hip -- the geometry of a loaded grid recomputed on the device from new node coordinates (nin_grid_update_points*).
//
// The connectivity stays; coords, centroids, face centres, float32 face normals and face areas are made again, bit for bit what
// grid_device.hip's k_centroids / k_faces_geometry (and grid_host.cpp, and the reference's calculate_centroids() +
// calculate_normal_faces(), grid.pyx:669-809) make of the same coordinates: divide-then-add in vertex order for the centroids,
// sum-then-divide for the face centres, float32 locals and sqrtf for the normals.  Compiled with -ffp-contract=off (build.py) like
// those two units: the reference is built without FMA.
//
// Those kernels run once per mesh; these run once per time step of a moving mesh and are bound by HBM traffic (at 216^3: 0.8 GB of
// indices in, 1.6 GB of records out, the coordinates mostly from the L2), so what matters is the shape of the accesses:
//   * one thread per cell / face; its index row is one aligned 32-byte (two dwordx4) / 16-byte (one dwordx4) load, so a wavefront
//     reads 2 KiB / 1 KiB of contiguous indices;
//   * the -1 padding of a row costs no divergent region (geom_math.hpp, which holds the per-cell and per-face arithmetic: the local
//     update of grid_scatter.hip compiles the same expressions);
//   * the 24-byte [..][3] double records and the 12-byte float normals of a workgroup go through LDS and leave as whole 16-byte
//     pieces per lane (a wavefront stores 1 KiB of contiguous bytes per instruction instead of 64 eight-byte pieces 24 bytes apart);
//     a workgroup's first record sits at 256 * 24 (or * 12) bytes times the block index: 16-byte aligned.
// Two kernels rather than one fused launch: the cells and the faces share no input row and no output, each fills the device on its
// own (tens of thousands of workgroups at 216^3), their LDS images differ, and separate launches keep separate lines in a kernel
// trace; the launch gap is microseconds against tenths of a millisecond of kernel.  The coordinates themselves are a device-to-device
// copy (coords_dim 3) or a small padding kernel (coords_dim 1, 2), enqueued first: both kernels read the grid's own [P][3] array.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "geom_math.hpp"
#include "launch.hpp"

namespace nin {

namespace {

constexpr int TPB = 256;

__global__ __launch_bounds__(TPB) void nin_update_pad_coords_kernel(int64_t P, int cd, const double *__restrict__ xyz,
                                                                     double *__restrict__ coords) {
    const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (p >= P) return;
    for (int k = 0; k < 3; ++k) coords[p * 3 + k] = k < cd ? xyz[p * cd + k] : 0.0;   // zero-padded, as k_ingest_coords
}

// s[0 .. 3 * TPB) holds the workgroup's records; `valid` of them are real.  A full workgroup stores 16 bytes per lane.
__device__ __forceinline__ void store_records_f64(const double *s, double *__restrict__ dst, int valid) {
    if (valid == TPB) {
        double2 *out = reinterpret_cast<double2 *>(dst);
        const double2 *in = reinterpret_cast<const double2 *>(s);
        out[threadIdx.x] = in[threadIdx.x];
        if (threadIdx.x < TPB / 2) out[TPB + threadIdx.x] = in[TPB + threadIdx.x];
    } else {   // the last workgroup of the launch
        for (int i = threadIdx.x; i < 3 * valid; i += TPB) dst[i] = s[i];
    }
}

__device__ __forceinline__ void store_records_f32(const float *s, float *__restrict__ dst, int valid) {
    if (valid == TPB) {
        if (threadIdx.x < 3 * TPB / 4) reinterpret_cast<float4 *>(dst)[threadIdx.x] = reinterpret_cast<const float4 *>(s)[threadIdx.x];
    } else {
        for (int i = threadIdx.x; i < 3 * valid; i += TPB) dst[i] = s[i];
    }
}

// npoel8: the points per cell of the eight element types, one byte each (type t in bits 8 t .. 8 t + 7)
__global__ __launch_bounds__(TPB) void nin_update_cells_kernel(int32_t E, int d, int32_t P, uint64_t npoel8, const int4 *__restrict__ inpoel,
                                                                const int8_t *__restrict__ etype, const double *__restrict__ X,
                                                                double *__restrict__ cen) {
    __shared__ __attribute__((aligned(16))) double s[3 * TPB];
    const int32_t e0 = (int32_t)blockIdx.x * TPB;
    const int32_t e = min(e0 + (int32_t)threadIdx.x, E - 1);   // lanes past the end redo the last cell; their records are not stored
    double c[3];
    cell_centroid_of(inpoel[2 * (int64_t)e], inpoel[2 * (int64_t)e + 1], npoel_of(npoel8, etype[e]), d, P, X, c);   // geom_math.hpp
#pragma unroll
    for (int k = 0; k < 3; ++k) s[3 * threadIdx.x + k] = c[k];
    __syncthreads();
    store_records_f64(s, cen + (int64_t)e0 * 3, min(TPB, E - e0));
}

template <bool DIM3>
__global__ __launch_bounds__(TPB) void nin_update_faces_kernel(int32_t F, int d, int32_t P, const int4 *__restrict__ inpofa,
                                                                const double *__restrict__ X, double *__restrict__ fc,
                                                                float *__restrict__ fn, double *__restrict__ fa) {
    __shared__ __attribute__((aligned(16))) double s[3 * TPB];
    __shared__ __attribute__((aligned(16))) float sn[3 * TPB];
    const int32_t f0 = (int32_t)blockIdx.x * TPB;
    const int32_t f = min(f0 + (int32_t)threadIdx.x, F - 1);
    double c[3], area;
    float nx, ny, nz;
    face_geometry_of<DIM3>(inpofa[f], d, P, X, c, nx, ny, nz, area);   // geom_math.hpp
#pragma unroll
    for (int k = 0; k < 3; ++k) s[3 * threadIdx.x + k] = c[k];
    sn[3 * threadIdx.x + 0] = nx; sn[3 * threadIdx.x + 1] = ny; sn[3 * threadIdx.x + 2] = nz;
    if (f0 + (int32_t)threadIdx.x < F) fa[f] = area;
    __syncthreads();
    const int valid = min(TPB, F - f0);
    store_records_f64(s, fc + (int64_t)f0 * 3, valid);
    store_records_f32(sn, fn + (int64_t)f0 * 3, valid);
}


}  // namespace

int launch_update_coords(const double *dev_xyz, int coords_dim, int64_t n_points, double *coords, hipStream_t stream) {
    if (n_points <= 0) return 0;
    if (coords_dim == 3)
        return launch_status(hipMemcpyAsync(coords, dev_xyz, (size_t)n_points * 24, hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(nin_update_pad_coords_kernel, blocks_for(n_points), dim3(TPB), 0, stream, n_points, coords_dim, dev_xyz, coords);
    return launch_status();
}

int launch_update_geometry(const GridView &g, uint64_t npoel8, const int32_t *inpoel, const int8_t *etype, const int32_t *inpofa,
                           double *centroids, double *face_center, float *face_normal, double *face_area, hipStream_t stream) {
    if (g.n_elems > 0)
        hipLaunchKernelGGL(nin_update_cells_kernel, blocks_for(g.n_elems), dim3(TPB), 0, stream, g.n_elems, (int)g.dim, g.n_points, npoel8,
                           reinterpret_cast<const int4 *>(inpoel), etype, g.coords, centroids);
    if (g.n_faces > 0) {
        if (g.dim == 3)
            hipLaunchKernelGGL((nin_update_faces_kernel<true>), blocks_for(g.n_faces), dim3(TPB), 0, stream, g.n_faces, 3, g.n_points,
                               reinterpret_cast<const int4 *>(inpofa), g.coords, face_center, face_normal, face_area);
        else
            hipLaunchKernelGGL((nin_update_faces_kernel<false>), blocks_for(g.n_faces), dim3(TPB), 0, stream, g.n_faces, (int)g.dim,
                               g.n_points, reinterpret_cast<const int4 *>(inpofa), g.coords, face_center, face_normal, face_area);
    }
    return launch_status();
}

}  // namespace nin
