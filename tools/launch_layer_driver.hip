// launch_layer_driver.hip -- the host side of the launch layer (csrc/launch.hpp) checked on a CPU: the chunk walk, the status of a launch
// and the grid of an uncapped kernel.  A stand-alone program with its own main, linked with the library's objects as
// `python -m ninpol_amd.build` left them (tests/test_launch_layer_host.py builds and runs it; tools/sanitize_gradop.sh takes it as its
// driver argument for a run under AddressSanitizer + UBSan).  Nothing is launched and nothing that opens a device is called: the program
// answers the same with and without a GPU.  One line per part, exit code 0 when every part is as expected.
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../ninpol_amd/csrc/launch.hpp"

static int failures = 0;

static void check(bool ok, const char *what, long long a = 0, long long b = 0) {
    if (ok) return;
    fprintf(stderr, "FAIL %s (%lld, %lld)\n", what, a, b);
    ++failures;
}

// for every n in 0 .. 9: the (NT, t0) pairs are the partition of [0, n) in order, every NT is MAX but a last one of n mod MAX, and a
// callback that answers 7 at its second call ends the walk there with 7
template <int MAX>
static void check_chunks() {
    const int before = failures;
    for (int32_t n = 0; n <= 9; ++n) {
        std::vector<std::pair<int, int32_t>> seen;
        const int rc = nin::for_each_chunk<MAX>(n, [&](auto nt, int32_t t0) {
            static_assert(decltype(nt)::value >= 1 && decltype(nt)::value <= MAX, "the chunk size is a compile-time constant in 1 .. MAX");
            seen.emplace_back(decltype(nt)::value, t0);
            return 0;
        });
        check(rc == 0, "a walk whose callback answers 0 returns 0", n, rc);
        check((int32_t)seen.size() == (n + MAX - 1) / MAX, "the number of chunks", n, (long long)seen.size());
        int32_t next = 0;
        for (size_t i = 0; i < seen.size(); ++i) {
            check(seen[i].second == next, "a chunk begins where the one before it ended", n, seen[i].second);
            const bool last = i + 1 == seen.size();
            check(seen[i].first == (last && n % MAX ? n % MAX : MAX), "the size of a chunk", n, seen[i].first);
            next += seen[i].first;
        }
        check(next == n, "the chunks cover [0, n)", n, next);

        int calls = 0;
        const int stopped = nin::for_each_chunk<MAX>(n, [&](auto, int32_t) { return ++calls == 2 ? 7 : 0; });
        const int chunks = (n + MAX - 1) / MAX;
        check(stopped == (chunks >= 2 ? 7 : 0), "the walk hands back the first non-zero answer", n, stopped);
        check(calls == (chunks >= 2 ? 2 : chunks), "no call follows a non-zero answer", n, calls);
    }
    printf("for_each_chunk<%d>: %s\n", MAX, failures == before ? "ok" : "FAILED");
}

static void check_status() {
    const int before = failures;
    check(nin::launch_status(hipSuccess) == 0, "launch_status(hipSuccess) is 0");
    const int rc = nin::launch_status(hipErrorInvalidConfiguration);
    check(rc == NIN_EHIP, "launch_status of an error is NIN_EHIP", rc, NIN_EHIP);
    const char *text = nin_last_error(), *words = hipGetErrorString(hipErrorInvalidConfiguration);
    if (!strstr(text, words)) {
        fprintf(stderr, "FAIL nin_last_error() is \"%s\", without HIP's \"%s\"\n", text, words);
        ++failures;
    }
    printf("launch_status: %s (\"%s\")\n", failures == before ? "ok" : "FAILED", text);
}

static void check_blocks() {
    const int before = failures;
    const int64_t big = ((int64_t)1 << 31) + 1;
    const struct { int64_t n; unsigned b256, b16; } want[] = {{0, 0, 0}, {1, 1, 1}, {256, 1, 16}, {257, 2, 17}, {big, (1u << 23) + 1, (1u << 27) + 1}};
    for (const auto &w : want) {
        const dim3 a = nin::blocks_for(w.n), a256 = nin::blocks_for(w.n, 256), a16 = nin::blocks_for(w.n, 16);
        check(a.x == w.b256 && a.y == 1 && a.z == 1, "blocks_for(n)", w.n, a.x);
        check(a256.x == w.b256 && a256.y == 1 && a256.z == 1, "blocks_for(n, 256)", w.n, a256.x);
        check(a16.x == w.b16 && a16.y == 1 && a16.z == 1, "blocks_for(n, 16)", w.n, a16.x);
    }
    printf("blocks_for: %s\n", failures == before ? "ok" : "FAILED");
}

int main() {
    check_chunks<4>();
    check_chunks<2>();
    check_status();
    check_blocks();
    printf("launch_layer_driver: %s\n", failures ? "FAILED" : "all answers as expected");
    return failures ? 1 : 0;
}
