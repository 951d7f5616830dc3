// base_classes_check.cpp -- CPU check of versalignlib_amd/csrc/base_classes.h (plain g++, no HIP; tests/test_base_classes.py
// builds and runs it): base_class4 gives base_class of every byte value at every byte of the dword, whatever its
// neighbours are; select_bytes8 is an eight-entry table; nonzero_bytes marks exactly the non-zero bytes.
#include <stdio.h>

#include <initializer_list>

#include "base_classes.h"

using namespace valign;

static int failures = 0;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++failures < 20) printf("FAILED line %d: %s\n", __LINE__, #cond); \
        }                                                                    \
    } while (0)

int main() {
    // the byte-wise rule itself: ten letters, nothing else
    int letters = 0;
    for (unsigned b = 0; b < 256; ++b) letters += base_class(b) != 0;
    CHECK(letters == 10);
    CHECK(base_class('A') == 1 && base_class('t') == 2 && base_class('C') == 3 && base_class('g') == 4 && base_class('N') == 5);
    CHECK(base_class('A' | 0x80) == 0 && base_class('a' | 0x80) == 0 && base_class(0) == 0 && base_class(0x20) == 0);

    // every byte value at every position, between neighbours that could carry or borrow into it
    const uint32_t neighbours[] = {0x00000000u, 0xFFFFFFFFu, 0x41414141u, 0x6E6E6E6Eu, 0x80808080u, 0x7F7F7F7Fu, 0x01010101u, 0x20202020u};
    for (uint32_t nb : neighbours)
        for (int pos = 0; pos < 4; ++pos)
            for (uint32_t b = 0; b < 256; ++b) {
                const uint32_t w = (nb & ~(0xFFu << (8 * pos))) | (b << (8 * pos));
                const uint32_t c = base_class4(w);
                for (int k = 0; k < 4; ++k) CHECK(((c >> (8 * k)) & 0xFFu) == (uint32_t)base_class((w >> (8 * k)) & 0xFFu));
            }
    // all pairs of byte values side by side (both orders are covered by the loop itself)
    for (uint32_t a = 0; a < 256; ++a)
        for (uint32_t b = 0; b < 256; ++b) {
            const uint32_t c = base_class4(a | b << 8 | a << 16 | b << 24);
            CHECK(c == ((uint32_t)base_class(a) * 0x00010001u | (uint32_t)base_class(b) * 0x01000100u));
        }

    for (uint32_t sel = 0; sel < 8; ++sel) {
        const uint32_t got = select_bytes8(0x77665544u, 0x33221100u, sel | (7 - sel) << 8 | sel << 16 | (sel ^ 1) << 24);
        CHECK(got == (sel * 0x11u | (7 - sel) * 0x11u << 8 | sel * 0x11u << 16 | (sel ^ 1) * 0x11u << 24));
    }
    for (uint32_t m = 0; m < 16; ++m)
        for (uint32_t v : {0x01u, 0x7Fu, 0x80u, 0xFFu}) {
            uint32_t w = 0, want = 0;
            for (int k = 0; k < 4; ++k)
                if (m >> k & 1) { w |= v << (8 * k); want |= 0x80u << (8 * k); }
            CHECK(nonzero_bytes(w) == want);
        }

    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("base classes ok\n");
    return 0;
}
