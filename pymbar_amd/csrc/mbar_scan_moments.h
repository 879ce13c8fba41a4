// ---- the host arithmetic of mbar_scan_moments (mbar_scan.cpp): buckets, slots, panel and record sizes, and the outputs by feature.
// Nothing here touches the device, so that a stand-alone program can run it under the host sanitizers
// (tools/scan_moments_host_check.cpp).
#pragma once
#include "mbar_scan.h"

#include <algorithm>
#include <vector>

namespace mbar {

// the smallest bucket that serves a family of B terms of which H are harmonic
inline ScanMoments scan_moments_bucket(int B, int H) {
    ScanMoments m;
    if (H == 0) m.bb = B <= 2 ? 2 : 8;
    else if (H <= 1 && B <= 3) m.hb = 1, m.bb = 3;
    else m.hb = 4, m.bb = 8;
    return m;
}

// The features of the C ABI in ascending b -- a linear term's basis, a harmonic term's dl then dl^2 -- and the slot of the kernel's
// bucket each one sits in (ScanMoments, mbar_scan.h).
inline std::vector<int> moment_slots(const FamilyTerms& terms, int B, const ScanMoments& mom) {
    std::vector<int> slot;
    int h = 0;
    for (int b = 0; b < B; ++b) {
        slot.push_back(mom.hb + b);
        if ((terms.mask >> b) & 1u) slot.push_back(h++);
    }
    return slot;
}

// what a call of L members over nchunks chunks needs: members per panel under the budget with the wider record, doubles of the
// partial records and of the merged outputs (M | lognum | out[L][record])
struct MomentSizes {
    int64_t panel;
    size_t part, out;
};
inline MomentSizes moment_sizes(int64_t budget_bytes, int64_t nchunks, int64_t record, int64_t L) {
    const int64_t pw = budget_bytes / (nchunks * record * (int64_t)sizeof(double)) / 64 * 64;
    MomentSizes z;
    z.panel = std::min<int64_t>(std::max<int64_t>(pw, 64), (L + 63) / 64 * 64);
    z.part = (size_t)nchunks * (size_t)record * (size_t)z.panel;
    z.out = (size_t)L * (size_t)(2 + record);
    return z;
}

// a member's merged sums by slot (out[record]) as the outputs of the C ABI, by feature
inline void moment_outputs(const double* out, int Q, const ScanMoments& mom, const std::vector<int>& slot, double* mean, double* m1, double* m2,
                    double* ma) {
    const int F = (int)slot.size(), FB = mom.slots(), NT = FB * (FB + 1) / 2;
    const double* A = out + 1 + Q;
    const double* Bt = A + FB;
    const double* C = Bt + NT;
    for (int j = 0; j <= Q; ++j) mean[j] = out[j];
    int k = 0;
    for (int i = 0; i < F; ++i) {
        m1[i] = A[slot[(size_t)i]];
        for (int j = i; j < F; ++j) {
            const int a = std::min(slot[(size_t)i], slot[(size_t)j]), b = std::max(slot[(size_t)i], slot[(size_t)j]);
            m2[k++] = Bt[a * FB - a * (a - 1) / 2 + (b - a)];  // row-major upper triangle of FB slots
        }
        for (int q = 0; q < Q; ++q) ma[q * F + i] = C[q * FB + slot[(size_t)i]];
    }
}

}  // namespace mbar
