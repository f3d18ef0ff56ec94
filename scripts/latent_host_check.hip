// latent_host_check.hip -- the host arithmetic of the latent-row entries as a stand-alone program for the sanitizers: row_parts and the
// three planners built on it over the corner inputs of tests/test_latent_plan.py, and place_ws / Bump against a malloc'd arena in
// place of the device workspace.  No GPU, no kernel launch: the planners are host functions of knn.hip, agg.hip and probe.hip.
//
//   cd argsim_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -fsanitize=address,undefined \
//       -I. ../../scripts/latent_host_check.hip knn.hip agg.hip probe.hip -o /tmp/latent_host_check && /tmp/latent_host_check
//
// The layout functions of the entries live inside their .cpp files; what runs here is place_ws itself with layouts of the same kinds
// (several element types, empty buffers, a start offset).
#include "ctx.h"
#include "row_parts.h"

#include <cstdio>
#include <cstdlib>

using namespace avae;
using namespace avae::host;

// the arena of this program: host memory (model.cpp's reserve_ws asks the device)
int avae::host::reserve_ws(avae_ctx* h, size_t need)
{
    if (need > ((size_t)1 << 40)) return 1;          // (refused like a size the device cannot give)
    if (need > h->ws_cap) {
        std::free(h->ws);
        h->ws = static_cast<char*>(std::malloc(need));
        h->ws_cap = h->ws ? need : 0;
    }
    return h->ws ? 0 : 1;
}

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static void check_parts(long long N, int tile, int max_parts, int chunk_opt, int parts, int chunk)
{
    if (N < 1) { EXPECT(parts == 0 && chunk == 0); return; }
    EXPECT(chunk >= 1 && chunk <= 0x7fffff80);
    EXPECT(parts == (int)((N + chunk - 1) / chunk) && parts >= 1 && parts <= max_parts);
    EXPECT(chunk_opt > 0 ? chunk >= std::min(chunk_opt, 0x7fffff80) : chunk % tile == 0);
    // what part_range does with the last part, in the kernels' types: begin + chunk in 64 bits, the end an int <= N
    const long long begin = (long long)(parts - 1) * chunk;
    EXPECT(begin < N && begin + chunk >= N);
}

struct Span { const char* p; size_t bytes; };
static void check_spans(const avae_ctx& h, const std::vector<Span>& spans, size_t from, size_t end)
{
    EXPECT(end + 4096 <= h.ws_cap);
    for (size_t i = 0; i < spans.size(); ++i) {
        const Span& s = spans[i];
        EXPECT(s.p != nullptr && ((uintptr_t)(s.p - h.ws) & 255) == 0);
        EXPECT(s.p >= h.ws + from && s.p + s.bytes <= h.ws + end);
        if (i) EXPECT(spans[i - 1].p + spans[i - 1].bytes <= s.p);
        for (size_t b = 0; b < s.bytes; b += 97) const_cast<char*>(s.p)[b] = 1;          // (the sanitizer sees a write beyond the arena)
        if (s.bytes) const_cast<char*>(s.p)[s.bytes - 1] = 1;
    }
}

int main()
{
    const long long Ns[] = {0, 1, 63, 64, 65, 127, 128, 129, 32767, 32768, 32769, 65535, 65536, 65537, 16255, 16256, 16257, 0x7fffffffLL - 255};
    const int opts[] = {0, 1, 50, 127, 128, 129, 1 << 30, 0x7fffffff}, ks[] = {1, 2, 16, 31, 32}, ns[] = {1, 32, 64, 65, 128, 129, 4096};
    long long plans = 0;
    for (long long N : Ns)
        for (int opt : opts) {
            for (int tile : {64, 128})
                for (int want : {0, 1, 8, 256, 1024})
                    for (int mp : {127, 256, 1024}) {
                        const RowParts r = row_parts(N, tile, want, mp, opt);
                        check_parts(N, tile, mp, opt, r.parts, r.chunk);
                        ++plans;
                    }
            for (int n : ns) {
                for (int k : ks) {
                    const KnnPlan p = knn_plan(n, (int)N, k, opt);
                    EXPECT((p.qrows == 32 || p.qrows == 128) && (long long)p.qtiles * p.qrows >= n);
                    check_parts(N, 128, std::min(512, 48 * 1024 / (12 * k) - 1), opt, p.parts, p.chunk);
                }
                if (N >= 1) { const AggPlan p = agg_plan(n, (int)N, 128, opt); EXPECT(p.qtiles * 128 >= n); check_parts(N, 64, 1024, opt, p.parts, p.chunk); }
            }
            if (N >= 1)
                for (int P : {1, 32, 33}) {
                    const ProbePlan p = probe_plan((int)N, P, 36, opt);
                    EXPECT(p.Ppad == p.ptiles * kProbeTile && p.Ppad >= P && p.Ppad < P + kProbeTile && p.LD == 40);
                    check_parts(N, 128, kProbeMaxParts, opt, p.parts, p.chunk);
                }
        }

    avae_ctx h;
    int placed = 0;
    for (size_t from : {(size_t)0, (size_t)1, (size_t)4096, (size_t)100001})
        for (size_t n : {(size_t)0, (size_t)1, (size_t)3, (size_t)257, (size_t)70000}) {
            std::vector<Span> spans;
            size_t end = 0;
            auto lay = [&](Bump& b) {
                spans.clear();
                float* f = b.take<float>(n);                       spans.push_back({(const char*)f, n * sizeof(float)});
                double* d = b.take<double>(3 * n + 1);             spans.push_back({(const char*)d, (3 * n + 1) * sizeof(double)});
                char* c = b.take<char>(n);                         spans.push_back({c, n});
                unsigned long long* u = b.take<unsigned long long>(0);      spans.push_back({(const char*)u, 0});
                int* on = b.opt<int>(true, n + 5);                 spans.push_back({(const char*)on, (n + 5) * sizeof(int)});
                EXPECT(b.opt<int>(false, n) == nullptr);
                float2* last = b.take<float2>(n * 2);              spans.push_back({(const char*)last, n * 2 * sizeof(float2)});
                end = b.off;
            };
            EXPECT(place_ws(&h, "check", lay, from) == 0);
            check_spans(h, spans, from, end);
            ++placed;
        }
    EXPECT(place_ws(&h, "check", [](Bump& b) { (void)b.take<char>(~(size_t)0 >> 1); }) == 1 && h.err.find("bytes") != std::string::npos);      // a refusal names its size
    EXPECT(check_rows(&h, "x", 8, "a and b", {h.ws, h.ws + 16}) == 0 && check_rows(&h, "x", 6, "a", {h.ws}) == 1 && check_rows(&h, "x", 8, "a and b", {h.ws, h.ws + 4}) == 1);
    EXPECT(h.err == "x: a and b must be 16-byte aligned");
    std::free(h.ws);
    std::printf("%lld row_parts plans, %d placements: %s\n", plans, placed, failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
