// ngs_utf8.h — the UTF-8 front end's codec: one decoding rule shared by the host
// (indexU8, single queries, the lazy key table) and the device decoder (ngs_utf8.hip).
//
// A string of bytes decodes into 32-bit units, left to right. Where a well-formed UTF-8 sequence
// (the Unicode standard's table: no overlong forms, no surrogates, nothing above U+10FFFF) starts
// and lies wholly inside the string, it yields its scalar value and takes 1-4 bytes. Any other
// byte b yields the unit 0x110000 + b alone: not a code point, so the wide normalisation turns it
// into a space, as the narrow API does with a byte outside validChar. The encoder is the total
// inverse (scalar -> UTF-8, 0x110000 + b -> byte b): encode(decode(s)) == s for every s.
//
// Plain C++17 without a HIP include: g++ compiles the host codec alone. Under hipcc the kernel
// launchers are declared too.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NGS_HD __host__ __device__
#else
#define NGS_HD
#endif

namespace ngs {

constexpr uint32_t kUtf8Invalid = 0x110000u;  // unit of an invalid byte b: kUtf8Invalid + b

// Length (1..4) of the well-formed UTF-8 sequence starting at p[0] with `avail` (>= 1) bytes
// left in the string; 0 if none starts there (a stray continuation byte, C0/C1, F5..FF, a second
// byte outside its lead's range, or a sequence cut short by the end of the string).
NGS_HD inline uint32_t utf8_wf_len(const uint8_t* p, size_t avail) {
    const uint32_t b0 = p[0];
    if (b0 < 0x80u) return 1;
    if (b0 < 0xC2u || b0 > 0xF4u) return 0;
    const uint32_t len = b0 < 0xE0u ? 2u : (b0 < 0xF0u ? 3u : 4u);
    if (avail < len) return 0;
    // the second byte's range depends on the lead (E0: A0..BF, ED: 80..9F, F0: 90..BF, F4: 80..8F)
    const uint32_t lo = b0 == 0xE0u ? 0xA0u : (b0 == 0xF0u ? 0x90u : 0x80u);
    const uint32_t hi = b0 == 0xEDu ? 0x9Fu : (b0 == 0xF4u ? 0x8Fu : 0xBFu);
    const uint32_t b1 = p[1];
    if (b1 < lo || b1 > hi) return 0;
    for (uint32_t k = 2; k < len; ++k)
        if ((p[k] & 0xC0u) != 0x80u) return 0;
    return len;
}

// The unit starting at p[0] given utf8_wf_len's answer for it (0: the invalid-byte unit).
NGS_HD inline uint32_t utf8_unit(const uint8_t* p, uint32_t wf) {
    const uint32_t b0 = p[0];
    switch (wf) {
        case 1: return b0;
        case 2: return ((b0 & 0x1Fu) << 6) | (p[1] & 0x3Fu);
        case 3: return ((b0 & 0x0Fu) << 12) | ((p[1] & 0x3Fu) << 6) | (p[2] & 0x3Fu);
        case 4: return ((b0 & 0x07u) << 18) | ((p[1] & 0x3Fu) << 12) | ((p[2] & 0x3Fu) << 6) | (p[3] & 0x3Fu);
        default: return kUtf8Invalid + b0;
    }
}

// Does a unit start at byte i of the string s[0, n)? The per-byte form of the rule (one lane per
// byte on the device): a byte that is not a continuation byte (80..BF) always starts one; a
// continuation byte starts one (as an invalid byte) unless the nearest non-continuation byte j
// with i - 3 <= j < i, inside the string, begins a well-formed sequence longer than i - j.
NGS_HD inline bool utf8_starts(const uint8_t* s, size_t n, size_t i) {
    if ((s[i] & 0xC0u) != 0x80u) return true;
    for (size_t k = 1; k <= 3 && k <= i; ++k) {
        const size_t j = i - k;
        if ((s[j] & 0xC0u) != 0x80u) return utf8_wf_len(s + j, n - j) <= k;
    }
    return true;
}

// Decodes s[0, n) into out (room for n units: a unit takes at least one byte); returns the number
// of units. out may be null to count only.
inline size_t utf8_decode(const uint8_t* s, size_t n, uint32_t* out) {
    size_t units = 0;
    for (size_t i = 0; i < n;) {
        const uint32_t wf = utf8_wf_len(s + i, n - i);
        if (out) out[units] = utf8_unit(s + i, wf);
        ++units;
        i += wf ? wf : 1;
    }
    return units;
}

// Bytes one unit encodes to. Units the decoder never yields (surrogates D800..DFFF and values
// above 0x1100FF, which only an indexW caller can put into a key) encode as U+FFFD.
inline uint32_t utf8_unit_len(uint32_t u) {
    if (u < 0x80u) return 1;
    if (u < 0x800u) return 2;
    if (u < 0x10000u) return 3;
    if (u < kUtf8Invalid) return 4;
    return u <= kUtf8Invalid + 0xFFu ? 1 : 3;
}

inline size_t utf8_encoded_len(const uint32_t* units, size_t n) {
    size_t bytes = 0;
    for (size_t i = 0; i < n; ++i) bytes += utf8_unit_len(units[i]);
    return bytes;
}

// Encodes n units into out (utf8_encoded_len bytes); returns the bytes written.
inline size_t utf8_encode(const uint32_t* units, size_t n, uint8_t* out) {
    uint8_t* o = out;
    for (size_t i = 0; i < n; ++i) {
        uint32_t u = units[i];
        if (u >= kUtf8Invalid) {
            if (u <= kUtf8Invalid + 0xFFu) {
                *o++ = (uint8_t)(u - kUtf8Invalid);
                continue;
            }
            u = 0xFFFDu;
        } else if (u >= 0xD800u && u <= 0xDFFFu) {
            u = 0xFFFDu;
        }
        if (u < 0x80u) {
            *o++ = (uint8_t)u;
        } else if (u < 0x800u) {
            *o++ = (uint8_t)(0xC0u | (u >> 6));
            *o++ = (uint8_t)(0x80u | (u & 0x3Fu));
        } else if (u < 0x10000u) {
            *o++ = (uint8_t)(0xE0u | (u >> 12));
            *o++ = (uint8_t)(0x80u | ((u >> 6) & 0x3Fu));
            *o++ = (uint8_t)(0x80u | (u & 0x3Fu));
        } else {
            *o++ = (uint8_t)(0xF0u | (u >> 18));
            *o++ = (uint8_t)(0x80u | ((u >> 12) & 0x3Fu));
            *o++ = (uint8_t)(0x80u | ((u >> 6) & 0x3Fu));
            *o++ = (uint8_t)(0x80u | (u & 0x3Fu));
        }
    }
    return (size_t)(o - out);
}

#if defined(__HIPCC__)
// Device decoder (ngs_utf8.hip): query i is the bytes raw8[off8[i] .. off8[i + 1]) (absolute
// offsets, any alignment, off8[0] need not be 0). Its units go to out32 from unit out_off[i] / 4:
// out_off[0 .. n] are BYTE offsets into out32 starting at 0 (4 x units; out_off[n] = total), the
// batch layout ngsSearchDevice takes for a wide index. A query whose units would end past
// out_cap_units is decoded as empty (and so is every query after it) and nothing of it is
// written; a capacity of off8[n] - off8[0] units always suffices. temp: utf8_temp_bytes(n) bytes
// of device scratch. Stream-ordered, no host wait.
size_t utf8_temp_bytes(uint32_t n);
hipError_t launch_utf8_decode(const uint8_t* raw8, const uint64_t* off8, uint32_t n, uint32_t* out32,
                              uint64_t out_cap_units, uint64_t* out_off, void* temp, size_t temp_bytes,
                              hipStream_t stream);
#endif

}  // namespace ngs
