// Host-side checks of ttsamd_stream_emit_resampled under the host sanitizers: a stand-alone program over csrc/stream_plan.hpp (the
// descriptor checks, the interval arithmetic with its int64 products, the by-value table, the tiling), which holds no HIP call.
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all tools/stream_plan_check.cpp -o /tmp/stream_plan_check
//   /tmp/stream_plan_check
// Every descriptor array is a heap block of exactly n_windows entries, so a read past one is an AddressSanitizer report.  Exit 0 and
// "ok" on the last line, or the first failed expectation.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../tts-arabic-pytorch_amd/csrc/stream_plan.hpp"

namespace ttsamd {
static char g_err[512];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
}  // namespace ttsamd

using namespace ttsamd;

#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, g_err); \
            return 1;                                                                  \
        }                                                                              \
    } while (0)

struct Win {
    int32_t start, len, utt, s0, s1;
};

static int32_t plan(const ResampleView& rv, const std::vector<Win>& wins, int W, int32_t w_max, int32_t hop, int32_t c_max, int32_t format,
                    EmitTable* tab, int32_t* nout) {
    const size_t m = wins.size();
    std::unique_ptr<int32_t[]> a(new int32_t[m]), b(new int32_t[m]), c(new int32_t[m]), d(new int32_t[m]), e(new int32_t[m]);
    for (size_t i = 0; i < m; ++i) {
        a[i] = wins[i].start; b[i] = wins[i].len; c[i] = wins[i].utt; d[i] = wins[i].s0; e[i] = wins[i].s1;
    }
    return stream_emit_plan(rv, W, w_max, hop, a.get(), b.get(), c.get(), d.get(), e.get(), c_max, format, tab, nout);
}

int main() {
    const int hop = 256;
    // (o, n, width) of 22 050 Hz -> 8 000, 16 000, 11 025, 44 100, 48 000 Hz at lowpass_filter_width 6, rolloff 0.99, and the NULL handle
    const int geo[][3] = {{441, 160, 17}, {441, 320, 9}, {2, 1, 13}, {1, 2, 7}, {147, 320, 7}, {1, 1, 0}};
    std::unique_ptr<EmitTable> tab(new EmitTable());
    for (const auto& g : geo) {
        const ResampleView rv{nullptr, g[0], g[1], g[2], 2 * g[2] + g[0], g[1]};
        const int reach = g[2] + g[0] - 1, halo = (reach + hop - 1) / hop;
        const EmitTiling t = emit_tiling(rv.o, rv.n);
        EXPECT(t.PC >= 1 && t.PC <= EMIT_THREADS && t.FR >= 1 && t.FR * t.PC <= EMIT_THREADS && t.PCH * t.PC >= rv.n);
        EXPECT(t.JC >= 1 && (t.FR - 1) * rv.o + t.JC <= EMIT_LDS);
        // every one-frame core of a 40-frame utterance with the smallest window the contract takes, and with one sample less per side
        const int T = 40;
        const int64_t L = (int64_t)hop * T;
        int64_t total = 0, next = 0;
        for (int f = 0; f < T; ++f) {
            const int32_t s0 = hop * f, s1 = hop * (f + 1);
            const int32_t ws = s0 - hop * halo > 0 ? s0 - hop * halo : 0;
            const int32_t we = s1 + hop * halo < L ? s1 + hop * halo : (int32_t)L;
            int32_t no = -1;
            EXPECT(plan(rv, {{ws, we - ws, (int32_t)L, s0, s1}}, 1, T, hop, 2 * hop * rv.n / rv.o + 2, 3, tab.get(), &no) == 0);
            EXPECT(tab->k0[0] == next && no == tab->nout[0] && no >= 0);
            EXPECT(tab->lo[0] >= ws && tab->hi[0] <= we && tab->lo[0] >= s0 - reach && tab->hi[0] <= s1 + reach);
            next += no;
            total += no;
            // the tight window, then one sample short on either side
            const int32_t lo = tab->lo[0] < s0 ? tab->lo[0] : s0, hi = tab->hi[0] > s1 ? tab->hi[0] : s1;
            if (no > 0) {
                EXPECT(plan(rv, {{lo, hi - lo, (int32_t)L, s0, s1}}, 1, T, hop, 4096, 0, tab.get(), nullptr) == 0);
                if (tab->lo[0] < s0) EXPECT(plan(rv, {{lo + 1, hi - lo - 1, (int32_t)L, s0, s1}}, 1, T, hop, 4096, 0, tab.get(), nullptr) == TTSAMD_EINVAL);
                if (tab->hi[0] > s1) EXPECT(plan(rv, {{lo, hi - lo - 1, (int32_t)L, s0, s1}}, 1, T, hop, 4096, 0, tab.get(), nullptr) == TTSAMD_EINVAL);
                int32_t keep = 12345;
                EXPECT(plan(rv, {{lo, hi - lo, (int32_t)L, s0, s1}}, 1, T, hop, no - 1 > 0 ? no - 1 : 1, 0, tab.get(), &keep) == (no > 1 ? TTSAMD_EINVAL : 0));
                EXPECT(no <= 1 || keep == 12345);                            // a refusal writes no count
            }
        }
        EXPECT(total == (rv.n * L + rv.o - 1) / rv.o);
    }
    // the int64 products: the largest ratio at the end of an utterance of 2^31 - 1 samples (n * S1 is about 2^43)
    {
        const ResampleView rv{nullptr, 4095, 4096, 7, 2 * 7 + 4095, 4096};
        const int32_t L = 0x7fffffff, s0 = L - 1000, s1 = L, ws = s0 - 8192;
        int32_t no = 0;
        EXPECT(plan(rv, {{ws, L - ws, L, s0, s1}}, 1, 1 << 20, 256, 2048, 2, tab.get(), &no) == 0);
        const int64_t k0 = (4096ll * s0 + 4094) / 4095, k1 = (4096ll * s1 + 4094) / 4095;
        EXPECT(tab->k0[0] == k0 && no == k1 - k0 && no > 1000 && tab->hi[0] == L);
    }
    // refusals before anything else is read: window counts, format, sizes, null arrays, inconsistent descriptors
    const ResampleView id{nullptr, 1, 1, 0, 1, 1};
    const std::vector<Win> one = {{0, 512, 512, 0, 256}};
    EXPECT(plan(id, one, 1, 2, 256, 256, 0, tab.get(), nullptr) == 0 && tab->nout[0] == 256 && tab->lo[0] == 0 && tab->hi[0] == 256);
    EXPECT(plan(id, one, 0, 2, 256, 256, 0, tab.get(), nullptr) == TTSAMD_EINVAL);
    EXPECT(plan(id, std::vector<Win>(65, one[0]), 65, 2, 256, 256, 0, tab.get(), nullptr) == TTSAMD_EINVAL);
    EXPECT(plan(id, std::vector<Win>(64, one[0]), 64, 2, 256, 256, 3, tab.get(), nullptr) == 0 && tab->nout[63] == 256);
    EXPECT(plan(id, one, 1, 2, 256, 256, 4, tab.get(), nullptr) == TTSAMD_EINVAL && plan(id, one, 1, 2, 256, 256, -1, tab.get(), nullptr) == TTSAMD_EINVAL);
    EXPECT(plan(id, one, 1, 2, 256, 255, 0, tab.get(), nullptr) == TTSAMD_EINVAL);                    // nout > c_max
    EXPECT(plan(id, one, 1, 1, 256, 256, 0, tab.get(), nullptr) == TTSAMD_EINVAL);                    // win_len > hop * w_max
    EXPECT(plan(id, {{0, 512, 255, 0, 256}}, 1, 2, 256, 256, 0, tab.get(), nullptr) == TTSAMD_EINVAL);  // core_end > utt_len
    EXPECT(plan(id, {{1, 511, 512, 0, 256}}, 1, 2, 256, 256, 0, tab.get(), nullptr) == TTSAMD_EINVAL);  // core before the window
    EXPECT(plan(id, {{0, 255, 512, 0, 256}}, 1, 2, 256, 256, 0, tab.get(), nullptr) == TTSAMD_EINVAL);  // core past the window
    EXPECT(plan(id, {{0, 512, 512, 256, 256}}, 1, 2, 256, 256, 0, tab.get(), nullptr) == TTSAMD_EINVAL);  // empty core
    EXPECT(plan(id, {{-1, 512, 512, 0, 256}}, 1, 2, 256, 256, 0, tab.get(), nullptr) == TTSAMD_EINVAL);
    EXPECT(plan(id, one, 1, 1 << 24, 256, 256, 0, tab.get(), nullptr) == TTSAMD_EINVAL);              // hop * w_max past 2^31
    EXPECT(stream_emit_plan(id, 1, 2, 256, nullptr, nullptr, nullptr, nullptr, nullptr, 256, 0, tab.get(), nullptr) == TTSAMD_EINVAL);
    std::printf("ok\n");
    return 0;
}
