// sanitize_gradop_driver.hip -- the host code of csrc/abi_gradop.hip under AddressSanitizer + UBSan on a CPU (tools/sanitize_gradop.sh builds
// abi_gradop.hip and this file with -Xarch_host -fsanitize=address,undefined and links them with the library's other objects).  No device
// is needed and none is touched: every call below is answered before the first HIP call -- the NULL arguments, the count, the dimension,
// the residency of a host-only grid -- on objects this program stands on host-only grids itself, and the sizing is exercised in 64-bit
// arithmetic at the node counts of 216^3 and 432^3 hexahedra.  Exit code 0: every answer is the expected one (the sanitizers abort on
// their own findings).
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

// sum_p 3 ne_p^2 of a box of N^3 hexahedra: along each axis two end nodes with one cell and N - 1 inner nodes with two, so the sum of
// ne^2 = (a b c)^2 over the nodes factorises into (2 * 1 + (N - 1) * 4)^3
static int64_t hex_values(int64_t N) {
    const int64_t per_axis = 2 + 4 * (N - 1);
    return 3 * per_axis * per_axis * per_axis;
}

int main() {
    nin_grid g3, g2;
    g3.h.dim = 3; g3.h.n_elems = 27; g3.h.n_points = 64;
    g2.h.dim = 2; g2.h.n_elems = 16; g2.h.n_points = 25;
    nin_gls_gradop op3, op2;   // never created by the library: no device buffers, nothing to destroy
    op3.g = &g3; op3.nnz = 216; op3.points = 64; op3.elems = 27;
    op2.g = &g2;
    std::vector<double> buf(4096, 0.0);
    double *b = buf.data();
    int64_t bytes = -7;
    nin_gls_gradop *made = &op3;

    const char *NUL = "NULL argument", *CNT = "n must be >= 1", *DIM = "the gradient operator is for 3-D grids only (this grid is 2-D)";
    const char *RES = "grid is not on a device: the kernels are HIP only", *FIRST = "grid is not on a device (call nin_grid_to_device first)";
    expect("bytes, NULL grid", nin_gls_gradop_bytes(nullptr, &bytes), NIN_EINVAL, NUL);
    expect("bytes, NULL out", nin_gls_gradop_bytes(&g3, nullptr), NIN_EINVAL, NUL);
    expect("bytes, 2-D", nin_gls_gradop_bytes(&g2, &bytes), NIN_EINVAL, DIM);
    expect("bytes, host-only grid", nin_gls_gradop_bytes(&g3, &bytes), NIN_ENODEVICE, FIRST);
    expect("create, NULL grid", nin_gls_gradop_create(nullptr, &made), NIN_EINVAL, NUL);
    if (made) { fprintf(stderr, "FAIL create did not clear its output\n"); ++failures; }
    expect("create, NULL out", nin_gls_gradop_create(&g3, nullptr), NIN_EINVAL, NUL);
    expect("create, 2-D", nin_gls_gradop_create(&g2, &made), NIN_EINVAL, DIM);
    expect("create, host-only grid", nin_gls_gradop_create(&g3, &made), NIN_ENODEVICE, FIRST);
    expect("factorize, NULL", nin_gls_gradop_factorize(nullptr, nullptr), NIN_EINVAL, NUL);
    expect("factorize, host-only grid", nin_gls_gradop_factorize(&op3, nullptr), NIN_ENODEVICE, RES);
    expect("factorize_host, host-only grid", nin_gls_gradop_factorize_host(&op3), NIN_ENODEVICE, RES);
    expect("apply, NULL object", nin_gls_gradop_apply(nullptr, 1, b, b, b, b, nullptr), NIN_EINVAL, NUL);
    expect("apply, NULL u", nin_gls_gradop_apply(&op3, 1, nullptr, b, b, b, nullptr), NIN_EINVAL, NUL);
    expect("apply, NULL grad", nin_gls_gradop_apply(&op3, 1, b, nullptr, b, b, nullptr), NIN_EINVAL, NUL);
    expect("apply, NULL before the count", nin_gls_gradop_apply(&op3, 0, nullptr, b, b, b, nullptr), NIN_EINVAL, NUL);
    expect("apply, n 0", nin_gls_gradop_apply(&op3, 0, b, b, nullptr, nullptr, nullptr), NIN_EINVAL, CNT);
    expect("apply, n < 0", nin_gls_gradop_apply(&op3, -2147483647 - 1, b, b, b, b, nullptr), NIN_EINVAL, CNT);
    expect("apply, the count before the dimension", nin_gls_gradop_apply(&op2, 0, b, b, b, b, nullptr), NIN_EINVAL, CNT);
    expect("apply, 2-D", nin_gls_gradop_apply(&op2, 1, b, b, b, b, nullptr), NIN_EINVAL, DIM);
    expect("apply, host-only grid", nin_gls_gradop_apply(&op3, 1, b, b, nullptr, nullptr, nullptr), NIN_ENODEVICE, RES);
    expect("transpose, NULL object", nin_gls_gradop_apply_transpose(nullptr, 1, b, b, nullptr), NIN_EINVAL, NUL);
    expect("transpose, NULL gbar", nin_gls_gradop_apply_transpose(&op3, 1, nullptr, b, nullptr), NIN_EINVAL, NUL);
    expect("transpose, NULL ubar", nin_gls_gradop_apply_transpose(&op3, 1, b, nullptr, nullptr), NIN_EINVAL, NUL);
    expect("transpose, n 0", nin_gls_gradop_apply_transpose(&op3, 0, b, b, nullptr), NIN_EINVAL, CNT);
    expect("transpose, 2-D", nin_gls_gradop_apply_transpose(&op2, 3, b, b, nullptr), NIN_EINVAL, DIM);
    expect("transpose, host-only grid", nin_gls_gradop_apply_transpose(&op3, 3, b, b, nullptr), NIN_ENODEVICE, RES);
    expect("apply_host, NULL grad", nin_gls_gradop_apply_host(&op3, 1, b, nullptr, b, b), NIN_EINVAL, NUL);
    expect("apply_host, n 0", nin_gls_gradop_apply_host(&op3, 0, b, b, b, b), NIN_EINVAL, CNT);
    expect("apply_host, host-only grid", nin_gls_gradop_apply_host(&op3, 2, b, b, b, b), NIN_ENODEVICE, RES);
    expect("transpose_host, NULL object", nin_gls_gradop_apply_transpose_host(nullptr, 1, b, b), NIN_EINVAL, NUL);
    expect("transpose_host, host-only grid", nin_gls_gradop_apply_transpose_host(&op3, 1, b, b), NIN_ENODEVICE, RES);
    expect("fetch_host, NULL gop_ptr", nin_gls_gradop_fetch_host(&op3, nullptr, b), NIN_EINVAL, NUL);
    expect("fetch_host, host-only grid", nin_gls_gradop_fetch_host(&op3, &bytes, b), NIN_ENODEVICE, RES);
    const int64_t *pp = nullptr;
    const double *pg = nullptr;
    int64_t nv = -1, sb = -1, stamp[3] = {0, 0, 0};
    expect("records, NULL object", nin_gls_gradop_records(nullptr, &pp, &pg, &nv, &sb), NIN_EINVAL, NUL);
    expect("records, NULL n_values", nin_gls_gradop_records(&op3, &pp, &pg, nullptr, &sb), NIN_EINVAL, NUL);
    expect("records", nin_gls_gradop_records(&op3, &pp, &pg, &nv, &sb), NIN_OK, nullptr);
    if (pp || pg || nv != 0 || sb != 8 * 65 + 4 * 216) { fprintf(stderr, "FAIL records: %lld %lld\n", (long long)nv, (long long)sb); ++failures; }
    expect("stamp, NULL", nin_gls_gradop_stamp(nullptr, stamp), NIN_EINVAL, NUL);
    expect("stamp", nin_gls_gradop_stamp(&op3, stamp), NIN_OK, nullptr);
    if (stamp[0] != -1 || stamp[1] != -1 || stamp[2] != -1) { fprintf(stderr, "FAIL the stamp of an object never factorised\n"); ++failures; }
    nin_gls_gradop_destroy(nullptr);
    if (bytes != -7) { fprintf(stderr, "FAIL a refused call wrote its output\n"); ++failures; }
    for (double v : buf)
        if (v != 0.0) { fprintf(stderr, "FAIL a refused call wrote into a buffer\n"); ++failures; break; }

    // the sizing: a node's block, and buffers of exactly the counted size take the last element of the documented layouts
    for (int64_t ne : {1, 2, 8, 24, 64}) {
        std::vector<double> block((size_t)nin::gradop_block_values(ne));
        block[(size_t)((ne - 1) * 3 * ne + 3 * ne - 1)] = 1.0;           // column ne - 1, row 3 ne - 1
        if (nin::gradop_block_values(ne) != 3 * ne * ne) { fprintf(stderr, "FAIL block of %lld cells\n", (long long)ne); ++failures; }
    }
    for (int32_t n : {1, 3, 4, 9}) {
        std::vector<double> dots(nin::gradop_dots_count(216, n));
        const int32_t chunk = n < nin::kGradopChunk ? n : nin::kGradopChunk;
        dots[(size_t)(chunk - 1) * 216 + 215] = 1.0;                      // dots [min(n, chunk)][nnz]
        if (dots.size() != (size_t)chunk * 216) { fprintf(stderr, "FAIL dots for %d fields\n", (int)n); ++failures; }
    }
    // 216^3 and 432^3 hexahedra: (216 + 1)^3 and (432 + 1)^3 nodes, 8 entries of esup per cell; every size is past 2^31, two past 2^33
    struct Big { int64_t N, values, gop_bytes; } bigs[] = {{216, 1921511784LL, 15372094272LL}, {432, 15425655528LL, 123405244224LL}};
    for (const Big &x : bigs) {
        const int64_t P = (x.N + 1) * (x.N + 1) * (x.N + 1), nnz = 8 * x.N * x.N * x.N;
        const nin::GradopBytes s = nin::gradop_bytes(hex_values(x.N), P, nnz);
        if (hex_values(x.N) != x.values || s.gop != x.gop_bytes || s.gop_ptr != 8 * (P + 1) || s.pos_node != 4 * nnz ||
            nin::gradop_dots_count(nnz, 7) != (size_t)4 * (size_t)nnz) {
            fprintf(stderr, "FAIL sizes at %lld^3: %lld values, %lld bytes\n", (long long)x.N, (long long)hex_values(x.N), (long long)s.gop);
            ++failures;
        }
    }
    printf("sanitize_gradop_driver: %s\n", failures ? "FAILED" : "all answers as expected");
    return failures ? 1 : 0;
}
