// sanitize_gradient_driver.hip -- the host code of csrc/abi_gradient.hip under AddressSanitizer + UBSan on a CPU (tools/sanitize_gradient.sh
// builds abi_gradient.hip and this file with -Xarch_host -fsanitize=address,undefined and links them with the library's other objects).
// No device is needed and none is touched: every call below is answered before the first HIP call -- the NULL arguments, the count, the
// dimension, the residency of a host-only grid -- and the buffer sizing is exercised by writing the last element of every buffer a
// caller would allocate from it.  Exit code 0: every answer is the expected one (the sanitizers abort on their own findings).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../ninpol_amd/csrc/abi_internal.hpp"

static int failures = 0;

static void expect(const char *what, int rc, int want_rc, const char *want_text) {
    const char *text = nin_last_error();
    if (rc != want_rc || (want_text && strcmp(text, want_text) != 0)) {
        fprintf(stderr, "FAIL %s: rc %d (want %d), text \"%s\"%s%s\n", what, rc, want_rc, text, want_text ? ", want " : "", want_text ? want_text : "");
        ++failures;
    }
}

int main() {
    // two host-only grids: the entry points read the host's dimension and the device's residency and nothing else of them
    nin_grid g3, g2;
    g3.h.dim = 3; g3.h.n_elems = 27; g3.h.n_points = 64;
    g2.h.dim = 2; g2.h.n_elems = 16; g2.h.n_points = 25;
    std::vector<double> buf(4096, 0.0);
    double *b = buf.data();

    const char *NUL = "NULL argument", *CNT = "n_fields must be >= 1", *DIM = "the corner gradients are for 3-D grids only (this grid is 2-D)";
    const char *RES = "grid is not on a device: the kernels are HIP only";
    expect("device, NULL grid", nin_gls_corner_gradients_device(nullptr, 1, b, b, b, b, b, nullptr), NIN_EINVAL, NUL);
    expect("device, NULL u", nin_gls_corner_gradients_device(&g3, 1, nullptr, b, b, b, b, nullptr), NIN_EINVAL, NUL);
    expect("device, NULL grad", nin_gls_corner_gradients_device(&g3, 1, b, nullptr, b, b, b, nullptr), NIN_EINVAL, NUL);
    expect("device, n_fields 0", nin_gls_corner_gradients_device(&g3, 0, b, b, b, b, b, nullptr), NIN_EINVAL, CNT);
    expect("device, n_fields < 0", nin_gls_corner_gradients_device(&g3, -2147483647 - 1, b, b, nullptr, nullptr, nullptr, nullptr), NIN_EINVAL, CNT);
    expect("device, 2-D", nin_gls_corner_gradients_device(&g2, 1, b, b, b, b, b, nullptr), NIN_EINVAL, DIM);
    expect("device, host-only grid", nin_gls_corner_gradients_device(&g3, 1, b, b, nullptr, nullptr, nullptr, nullptr), NIN_ENODEVICE, RES);
    expect("host, NULL grid", nin_gls_corner_gradients_host(nullptr, b, 1, b, b, b, b), NIN_EINVAL, NUL);
    expect("host, NULL values", nin_gls_corner_gradients_host(&g3, nullptr, 1, b, b, b, b), NIN_EINVAL, NUL);
    expect("host, NULL grad", nin_gls_corner_gradients_host(&g3, b, 1, nullptr, b, b, b), NIN_EINVAL, NUL);
    expect("host, n_fields 0", nin_gls_corner_gradients_host(&g3, b, 0, b, b, b, b), NIN_EINVAL, CNT);
    expect("host, 2-D", nin_gls_corner_gradients_host(&g2, b, 3, b, nullptr, nullptr, nullptr), NIN_EINVAL, DIM);
    expect("host, host-only grid", nin_gls_corner_gradients_host(&g3, b, 3, b, b, b, b), NIN_ENODEVICE, RES);
    for (double v : buf)
        if (v != 0.0) { fprintf(stderr, "FAIL a refused call wrote into a buffer\n"); ++failures; break; }

    // the sizing: buffers of exactly the counted size take the last element of the documented layouts; and at the size of 216^3
    // hexahedra with twelve fields the counts are those of 64-bit arithmetic (grad passes 2^31 doubles)
    const int64_t E = 27, P = 64, nnz = 216;
    for (int32_t k : {1, 3}) {
        const nin::CornerGradientCounts n = nin::corner_gradient_counts(E, P, nnz, k);
        std::vector<double> u(n.u), grad(n.grad), vals(n.node_values), ng(n.node_gradient);
        u[(size_t)(k - 1) * E + (E - 1)] = 1.0;                      // u [k][E]
        grad[((size_t)(k - 1) * nnz + (nnz - 1)) * 3 + 2] = 1.0;     // grad, flux [k][nnz][3]
        vals[(size_t)(k - 1) * P + (P - 1)] = 1.0;                   // node_values [k][P]
        ng[((size_t)(k - 1) * P + (P - 1)) * 3 + 2] = 1.0;           // node_gradient [k][P][3]
        if (n.u != (size_t)k * 27 || n.grad != (size_t)k * 216 * 3 || n.node_values != (size_t)k * 64 || n.node_gradient != (size_t)k * 64 * 3) {
            fprintf(stderr, "FAIL counts for %d fields\n", (int)k);
            ++failures;
        }
    }
    const nin::CornerGradientCounts big = nin::corner_gradient_counts(10077696, 10218313, 80621568, 12);
    if (big.grad != (size_t)2902376448 || big.u != (size_t)120932352 || big.node_gradient != (size_t)367859268) {
        fprintf(stderr, "FAIL counts at 216^3: %zu %zu %zu\n", big.grad, big.u, big.node_gradient);
        ++failures;
    }
    printf("sanitize_gradient_driver: %s\n", failures ? "FAILED" : "all answers as expected");
    return failures ? 1 : 0;
}
