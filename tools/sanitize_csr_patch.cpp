// sanitize_csr_patch.cpp -- nin_csr_patch_rows (ninpol_amd/csrc/csr_patch.cpp) under the host sanitizers, as a program of its own:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/sanitize_csr_patch.cpp ninpol_amd/csrc/csr_patch.cpp -o tools/_bin/csr_patch_asan && tools/_bin/csr_patch_asan
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=thread \
//       tools/sanitize_csr_patch.cpp ninpol_amd/csrc/csr_patch.cpp -o tools/_bin/csr_patch_tsan && tools/_bin/csr_patch_tsan
//
// (no GPU, no ROCm: the header is plain C and csr_patch.cpp is OpenMP only.  libgomp is not built for ThreadSanitizer, which cannot
// see its fork, join and barriers and reports the hand-over of every array to a parallel region as a race; for a run that means
// something use a compiler whose OpenMP runtime ThreadSanitizer understands -- clang++ with libomp and its archer tool -- with
// TSAN_OPTIONS=ignore_noninstrumented_modules=1.)
// Every array is allocated at its exact size, so a read or write one element outside is an AddressSanitizer report; the results are
// compared with a serial model.  Random CSR matrices of P = 1, 63, 64, 65, 1000 and 20000 rows of 0 .. 90 entries; the patched rows in
// random order; in place (equal counts, other pattern), into out_* (rows growing, shrinking, emptied, filled), and the refusals.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../include/ninpol_amd.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {   // 0 .. n - 1
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % (n ? n : 1));
}

struct Csr {
    std::vector<int32_t> indptr, indices;
    std::vector<double> data;
};

Csr make(const std::vector<int32_t> &len) {
    Csr c;
    c.indptr.assign(len.size() + 1, 0);
    for (size_t p = 0; p < len.size(); ++p) c.indptr[p + 1] = c.indptr[p] + len[p];
    c.indices.resize((size_t)c.indptr.back());
    c.data.resize((size_t)c.indptr.back());
    for (size_t i = 0; i < c.indices.size(); ++i) { c.indices[i] = (int32_t)rnd(100000); c.data[i] = 1.0 + rnd(1000) * 0.001; }
    return c;
}

int g_failures = 0;
void expect(bool ok, const char *what, int64_t P) {
    if (!ok) { ++g_failures; fprintf(stderr, "FAILED: %s (P = %lld)\n", what, (long long)P); }
}

void one_size(int64_t P) {
    std::vector<int32_t> len((size_t)P);
    for (auto &l : len) l = (int32_t)rnd(91);
    const Csr A = make(len);
    std::vector<double> nws((size_t)P, 0.5);
    for (int m_kind = 0; m_kind < 3; ++m_kind) {
        const int64_t m = m_kind == 0 ? 0 : m_kind == 1 ? 1 : P;
        std::vector<int32_t> nodes((size_t)P);
        std::iota(nodes.begin(), nodes.end(), 0);
        for (int64_t i = P - 1; i > 0; --i) std::swap(nodes[(size_t)i], nodes[rnd((uint32_t)i + 1)]);
        nodes.resize((size_t)m);
        for (int reshape = 0; reshape < 2; ++reshape) {
            std::vector<int32_t> cnt((size_t)m);
            for (int64_t i = 0; i < m; ++i) {
                const int32_t k = len[(size_t)nodes[(size_t)i]];
                cnt[(size_t)i] = !reshape ? k : (i % 4 == 0 ? (k < 90 ? k + 1 : k) : i % 4 == 1 ? (k ? k - 1 : 0) : i % 4 == 2 ? 0 : (k ? k : 3));
            }
            const Csr pk = make(cnt);
            std::vector<double> pnws((size_t)m, 2.0);
            // the serial model
            std::vector<int32_t> new_len(len);
            for (int64_t i = 0; i < m; ++i) new_len[(size_t)nodes[(size_t)i]] = cnt[(size_t)i];
            Csr want = make(new_len);
            std::vector<int64_t> from((size_t)P, -1);
            for (int64_t i = 0; i < m; ++i) from[(size_t)nodes[(size_t)i]] = i;
            for (int64_t p = 0; p < P; ++p)
                for (int32_t j = 0; j < new_len[(size_t)p]; ++j) {
                    const int64_t i = from[(size_t)p];
                    const size_t src = (size_t)(i < 0 ? A.indptr[(size_t)p] : pk.indptr[(size_t)i]) + (size_t)j, dst = (size_t)want.indptr[(size_t)p] + (size_t)j;
                    want.indices[dst] = i < 0 ? A.indices[src] : pk.indices[src];
                    want.data[dst] = i < 0 ? A.data[src] : pk.data[src];
                }
            Csr B = A;
            std::vector<double> bn(nws);
            // size-0 vectors: data() may be null, and NULL is refused -- one spare element behind the arrays that can be empty
            B.indices.reserve(B.indices.size() + 1); B.data.reserve(B.data.size() + 1);
            Csr pkc = pk;
            pkc.indices.reserve(pkc.indices.size() + 1); pkc.data.reserve(pkc.data.size() + 1);
            nodes.reserve(nodes.size() + 1); cnt.reserve(cnt.size() + 1); pnws.reserve(pnws.size() + 1);
            if (!reshape) {
                const int rc = nin_csr_patch_rows(P, B.indptr.data(), B.indices.data(), B.data.data(), bn.data(), m, nodes.data(), cnt.data(),
                                                  pkc.indptr.data(), pkc.indices.data(), pkc.data.data(), pnws.data(), nullptr, nullptr, nullptr);
                expect(rc == NIN_OK && B.indices == want.indices && B.data == want.data, "in place", P);
            } else {
                Csr O;
                O.indptr.assign((size_t)P + 1, -7);
                O.indices.assign(want.indices.size(), -7);
                O.data.assign(want.data.size(), -7.0);
                O.indices.reserve(O.indices.size() + 1); O.data.reserve(O.data.size() + 1);
                const int rc = nin_csr_patch_rows(P, B.indptr.data(), B.indices.data(), B.data.data(), bn.data(), m, nodes.data(), cnt.data(),
                                                  pkc.indptr.data(), pkc.indices.data(), pkc.data.data(), pnws.data(), O.indptr.data(), O.indices.data(),
                                                  O.data.data());
                expect(rc == NIN_OK && O.indptr == want.indptr && O.indices == want.indices && O.data == want.data, "out_*", P);
                expect(B.indices == A.indices && B.data == A.data, "out_*: the old matrix is an input", P);
            }
            for (int64_t i = 0; i < m; ++i) expect(bn[(size_t)nodes[(size_t)i]] == 2.0, "neumann_ws", P);
            if (m >= 1) {   // the refusals: nothing may be read outside the arrays on the way to them
                std::vector<int32_t> bad(nodes);
                bad[0] = (int32_t)P;
                expect(nin_csr_patch_rows(P, B.indptr.data(), B.indices.data(), B.data.data(), bn.data(), m, bad.data(), cnt.data(), pkc.indptr.data(),
                                          pkc.indices.data(), pkc.data.data(), pnws.data(), nullptr, nullptr, nullptr) == NIN_EINVAL, "node == P", P);
                bad[0] = -1;
                expect(nin_csr_patch_rows(P, B.indptr.data(), B.indices.data(), B.data.data(), bn.data(), m, bad.data(), cnt.data(), pkc.indptr.data(),
                                          pkc.indices.data(), pkc.data.data(), pnws.data(), nullptr, nullptr, nullptr) == NIN_EINVAL, "node == -1", P);
                if (m >= 2) {
                    bad[0] = nodes[1];
                    expect(nin_csr_patch_rows(P, B.indptr.data(), B.indices.data(), B.data.data(), bn.data(), m, bad.data(), cnt.data(), pkc.indptr.data(),
                                              pkc.indices.data(), pkc.data.data(), pnws.data(), nullptr, nullptr, nullptr) == NIN_EINVAL, "duplicate", P);
                }
                std::vector<int32_t> off(pkc.indptr);
                off[(size_t)m] += 1;
                expect(nin_csr_patch_rows(P, B.indptr.data(), B.indices.data(), B.data.data(), bn.data(), m, nodes.data(), cnt.data(), off.data(),
                                          pkc.indices.data(), pkc.data.data(), pnws.data(), nullptr, nullptr, nullptr) == NIN_EINVAL, "off", P);
                expect(nin_csr_patch_rows(P, B.indptr.data(), B.indices.data(), B.data.data(), bn.data(), m, nullptr, cnt.data(), pkc.indptr.data(),
                                          pkc.indices.data(), pkc.data.data(), pnws.data(), nullptr, nullptr, nullptr) == NIN_EINVAL, "NULL", P);
            }
        }
    }
}

}  // namespace

int main() {
    for (int64_t P : {1, 63, 64, 65, 1000, 20000}) one_size(P);
    if (g_failures) { fprintf(stderr, "%d checks failed\n", g_failures); return 1; }
    printf("nin_csr_patch_rows: all checks passed\n");
    return 0;
}
