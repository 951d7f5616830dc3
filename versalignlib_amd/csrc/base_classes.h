// base_classes.h -- the class of an input byte (A/a 1, T/t 2, C/c 3, G/g 4, N/n 5, else 0), one byte at a time and four
// bytes of a dword at a time.  Plain integer code: the kernels' set-up (dp_kernels.hip.h: wave_setup) uses the dword form,
// tests/base_classes_check.cpp compares the two for every byte value on the CPU.  No HIP here but the one builtin below.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VALIGN_HD __host__ __device__
#else
#define VALIGN_HD
#endif

namespace valign {

// base class of one input byte: A/a 1, T/t 2, C/c 3, G/g 4, N/n 5, else 0
VALIGN_HD inline int base_class(unsigned ch) {
    const unsigned u = ch & 0xDFu;            // fold case; bytes >= 0x80 never match
    int c = 0;
    c = (u == 'A') ? 1 : c;
    c = (u == 'T') ? 2 : c;
    c = (u == 'C') ? 3 : c;
    c = (u == 'G') ? 4 : c;
    c = (u == 'N') ? 5 : c;
    return c;
}

// Byte i of the result is byte (sel_i & 7) of the eight bytes {hi, lo} (0..3: lo, 4..7: hi) -- an eight-entry table
// looked up by four selectors at once.  Every selector byte must be 0..7.  One v_perm_b32 on the device.
VALIGN_HD inline uint32_t select_bytes8(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t table = ((uint64_t)hi << 32) | lo;
    uint32_t out = 0;
    for (int i = 0; i < 4; ++i) out |= (uint32_t)((table >> (8 * ((sel >> (8 * i)) & 7u))) & 0xFFu) << (8 * i);
    return out;
#endif
}

// 0x80 in every byte of v that is not zero, 0 in the others (exact: no carry leaves a byte)
VALIGN_HD inline uint32_t nonzero_bytes(uint32_t v) {
    return (((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u;
}

// base_class() of the four bytes of w, byte for byte.  Bits 1..3 of a case-folded letter tell the five letters apart
// (A 0, C 1, T 2, G 3, N 7): they pick the one letter the byte could be and that letter's class from two eight-entry
// tables; the class stays where the folded byte IS that letter.  (Table entries 4..6 hold 0x20, which no folded byte
// equals.)
VALIGN_HD inline uint32_t base_class4(uint32_t w) {
    const uint32_t u = w & 0xDFDFDFDFu;
    const uint32_t sel = (w >> 1) & 0x07070707u;
    const uint32_t letter = select_bytes8(0x4E202020u, 0x47544341u, sel);     // N . . . | G T C A
    const uint32_t cls = select_bytes8(0x05000000u, 0x04020301u, sel);
    const uint32_t differs = nonzero_bytes(u ^ letter);
    const uint32_t clear = (differs << 1) - (differs >> 7);                    // 0xFF in every byte that is no letter
    return cls & ~clear;
}

}  // namespace valign
