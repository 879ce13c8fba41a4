// Stand-alone check of the host arithmetic of mbar_scan_moments (pymbar_amd/csrc/mbar_scan_moments.h): the bucket a family gets, the
// slot of every feature, the panel and record sizes under every budget, and the scatter of a member's merged sums into the outputs
// of the C ABI.  No device: build it with the host sanitizers and run it on the CPU,
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all --offload-host-only \
//         -x hip tools/scan_moments_host_check.cpp -o /tmp/scan_moments_host_check && /tmp/scan_moments_host_check
// Every buffer is allocated at exactly the size the C ABI documents, so that an index one past an end is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>

#include "../pymbar_amd/csrc/mbar_scan_moments.h"

using namespace mbar;

#define REQUIRE(x)                                                    \
    do {                                                              \
        if (!(x)) {                                                   \
            std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

int main() {
    int families = 0;
    for (int B = 1; B <= SCAN_MAX_B; ++B)
        for (uint32_t mask = 0; mask < (1u << B); ++mask) {
            const int H = __builtin_popcount(mask);
            if (H > SCAN_MAX_H) continue;
            ++families;
            FamilyTerms terms;
            terms.mask = mask;
            const ScanMoments mom = scan_moments_bucket(B, H);
            const int F = B + H, FB = mom.slots(), NT = F * (F + 1) / 2;
            REQUIRE(B <= mom.bb && H <= mom.hb && (H == 0) == (mom.hb == 0) && FB <= SCAN_MAX_B + SCAN_MAX_H);
            const std::vector<int> slot = moment_slots(terms, B, mom);
            REQUIRE((int)slot.size() == F);
            REQUIRE((int)std::set<int>(slot.begin(), slot.end()).size() == F);  // no two features share a slot
            for (int s : slot) REQUIRE(s >= 0 && s < FB);
            for (int Q = 0; Q <= SCAN_MAX_Q; ++Q) {
                const int R = mom.record(Q);
                // a member's merged sums, every entry its own index; outputs at the documented sizes
                std::unique_ptr<double[]> out(new double[R]);
                for (int r = 0; r < R; ++r) out[r] = r;
                std::unique_ptr<double[]> mean(new double[1 + Q]), m1(new double[F]), m2(new double[NT]), ma(new double[Q * F > 0 ? Q * F : 1]);
                moment_outputs(out.get(), Q, mom, slot, mean.get(), m1.get(), m2.get(), Q ? ma.get() : nullptr);
                std::set<int> used;
                for (int j = 0; j <= Q; ++j) REQUIRE(mean[j] == j);
                int k = 0;
                for (int i = 0; i < F; ++i) {
                    REQUIRE(m1[i] == 1 + Q + slot[(size_t)i]);
                    for (int j = i; j < F; ++j) {
                        const int r = (int)m2[k++];
                        REQUIRE(r >= 1 + Q + FB && r < 1 + Q + FB + FB * (FB + 1) / 2 && used.insert(r).second);
                    }
                    for (int q = 0; q < Q; ++q) REQUIRE(ma[q * F + i] == 1 + Q + FB + FB * (FB + 1) / 2 + q * FB + slot[(size_t)i]);
                }
                // the diagonal of feature i is the diagonal of its slot
                k = 0;
                for (int i = 0; i < F; ++i) {
                    const int a = slot[(size_t)i];
                    REQUIRE(m2[k] == 1 + Q + FB + a * FB - a * (a - 1) / 2);
                    k += F - i;
                }
                // panels and buffers: a multiple of 64 members, at least 64, never more than the call rounds up to; the records of a
                // panel fit the budget unless a single panel of 64 does not
                for (int64_t budget : {(int64_t)1, (int64_t)1 << 20, (int64_t)1 << 28, (int64_t)1 << 40})
                    for (int64_t nchunks : {(int64_t)1, (int64_t)3, (int64_t)1954})
                        for (int64_t L : {(int64_t)1, (int64_t)64, (int64_t)65, (int64_t)130, (int64_t)100000}) {
                            const MomentSizes z = moment_sizes(budget, nchunks, R, L);
                            REQUIRE(z.panel >= 64 && z.panel % 64 == 0 && z.panel <= (L + 63) / 64 * 64);
                            REQUIRE(z.part == (size_t)nchunks * (size_t)R * (size_t)z.panel && z.out == (size_t)L * (size_t)(2 + R));
                            REQUIRE(z.panel == 64 || (int64_t)(z.part * sizeof(double)) <= budget);
                            // the last record entry a kernel of the panel writes, and the last merged entry, lie inside
                            const int64_t pl = L < z.panel ? L : z.panel;
                            REQUIRE((size_t)(((nchunks - 1) * R + (R - 1)) * pl + (pl - 1)) < z.part);
                            REQUIRE((size_t)(2 * L + (L - 1) * R + (R - 1)) < z.out);
                        }
            }
        }
    std::printf("scan_moments host check: %d families, ok\n", families);
    return 0;
}
