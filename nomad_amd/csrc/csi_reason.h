// What CSIVolumeChecker.Feasible records for a node it fails (feasible.go:251-259):
// FilterNode(node, reason), the reason one of seven texts built from the
// request, its volume and, for the plugin reasons, the node (feasible.go:19-26).
//
// pe_place_csi_metrics' kernel (k_csi_loop<true>) logs one byte per consumed
// visit position; the host turns a non-zero byte into the reason text. Both
// sides pack and unpack the byte with these lines, and the formatter is the one
// pe_csi_reason_text exposes.
//
// The byte: 0 for a position that does not fail the checker, else the 7-bit
// availability code of the placement's column (request index << 3 | reason,
// request < 16, reason 1..7) with bit 7 set when the kernel treated the node as
// a stop (its class memoised eligible: FeasibilityWrapper.Next returns nil,
// feasible.go:1112-1119) rather than a skip (:1145-1149).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#if defined(__HIP__)   // compiled as HIP (kernels.hip); plain C++ elsewhere
#define PE_CSI_REASON_HD __host__ __device__ __forceinline__
#else
#define PE_CSI_REASON_HD inline
#endif

namespace pe {

constexpr uint32_t kCsiLogStop = 0x80u;
constexpr uint32_t kCsiLogCodeMask = 0x7Fu;
constexpr uint64_t kCsiLogCap = 1ull << 24;   // bytes of one call's trace log

// code: 0, or request << 3 | reason as k_csi_avail stores it.
PE_CSI_REASON_HD uint8_t csi_log_pack(uint32_t code, bool stop) {
    const uint32_t c = code & kCsiLogCodeMask;
    return (uint8_t)(c ? (c | (stop ? kCsiLogStop : 0u)) : 0u);
}

PE_CSI_REASON_HD uint32_t csi_log_request(uint8_t b) { return (b & kCsiLogCodeMask) >> 3; }
PE_CSI_REASON_HD uint32_t csi_log_reason(uint8_t b) { return b & 7u; }
PE_CSI_REASON_HD bool csi_log_stop(uint8_t b) { return (b & kCsiLogStop) != 0; }

// The reason text (reason 1..7) into buf (at most cap bytes, NUL-terminated
// when cap > 0). Returns the bytes needed including the NUL, or -1 for a reason
// out of range. plugin / node_id are read for reasons 2 to 4 only, volume (the
// request's source after the per_alloc suffix, which is the volume's id where
// one was found) for the others; a null string reads as "".
inline int64_t csi_reason_text(uint32_t reason, const char* plugin, const char* volume, const char* node_id, char* buf,
                               size_t cap) {
    static const char* const kText[8] = {
        nullptr,
        "missing CSI Volume %s",
        "CSI plugin %s is missing from client %s",
        "CSI plugin %s is unhealthy on client %s",
        "CSI plugin %s has the maximum number of volumes on client %s",
        "CSI volume %s is unschedulable or has exhausted its available reader claims",
        "CSI volume %s is unschedulable or is read-only",
        "CSI volume %s has exhausted its available writer claims",
    };
    if (reason < 1u || reason > 7u) return -1;
    plugin = plugin ? plugin : "";
    volume = volume ? volume : "";
    node_id = node_id ? node_id : "";
    char none[1];
    char* dst = (buf && cap) ? buf : none;
    const size_t lim = (buf && cap) ? cap : 0;
    int n;
    if (reason >= 2u && reason <= 4u) n = snprintf(dst, lim, kText[reason], plugin, node_id);
    else n = snprintf(dst, lim, kText[reason], volume);
    return n < 0 ? -1 : (int64_t)n + 1;
}

}  // namespace pe
