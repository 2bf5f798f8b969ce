// Drives the argument checks of mi355_reverse_axes (csrc/resident_case.hip) on the host, for a sanitizer build: every refusal
// the entry point makes, then one call that passes them all.  No device is needed: a refusal returns before anything touches
// the HIP runtime, and the call that passes the checks ends at the device binding (MI355_ERR_NO_DEVICE on a machine without a
// GPU; on one with a gfx950 it runs the 2 x 3 x 4 x 5 reversal of the two host-invisible buffers below and is not looked at).
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//       -x hip tools/reverse_axes_refusals.cpp <pkg>/csrc/resident_case.hip <pkg>/csrc/runtime.hip -fsanitize=address,undefined -o reverse_axes_refusals
//   ./reverse_axes_refusals        (exit status 0 and "all refusals as expected")
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "mi355_nnunet.h"

static int failures = 0;

static void expect(const char *what, int rc, int want_rc, const char *want_text) {
    const char *msg = mi355_last_error();
    const bool ok = rc == want_rc && (!want_text || (msg && strstr(msg, want_text)));
    printf("%-44s rc %2d  %s\n", what, rc, rc < 0 && msg ? msg : "");
    if (!ok) {
        printf("  EXPECTED rc %d and a message with \"%s\"\n", want_rc, want_text ? want_text : "");
        ++failures;
    }
}

int main() {
    // two address ranges that are never dereferenced on the host: the entry point compares addresses only
    alignas(16) static unsigned char a[4 * 2 * 3 * 4 * 5 + 8], b[4 * 2 * 3 * 4 * 5 + 8];
    void *src = a, *dst = b;
    const int E = MI355_ERR_INVALID;
    expect("null source", mi355_reverse_axes(nullptr, dst, 2, 3, 4, 5, 4, nullptr), E, "null pointer");
    expect("null destination", mi355_reverse_axes(src, nullptr, 2, 3, 4, 5, 4, nullptr), E, "null pointer");
    expect("no channel", mi355_reverse_axes(src, dst, 0, 3, 4, 5, 4, nullptr), E, "bad shape");
    expect("d0 = 0", mi355_reverse_axes(src, dst, 2, 0, 4, 5, 4, nullptr), E, "bad shape");
    expect("d1 = INT_MIN", mi355_reverse_axes(src, dst, 2, 3, INT_MIN, 5, 4, nullptr), E, "bad shape");
    expect("d2 = -1", mi355_reverse_axes(src, dst, 2, 3, 4, -1, 4, nullptr), E, "bad shape");
    expect("2 bytes per element", mi355_reverse_axes(src, dst, 2, 3, 4, 5, 2, nullptr), E, "bytes per element");
    expect("0 bytes per element", mi355_reverse_axes(src, dst, 2, 3, 4, 5, 0, nullptr), E, "bytes per element");
    expect("-4 bytes per element", mi355_reverse_axes(src, dst, 2, 3, 4, 5, -4, nullptr), E, "bytes per element");
    expect("2^31 elements", mi355_reverse_axes(src, dst, 1, 2048, 1024, 1024, 1, nullptr), E, "2^31 elements or more");
    expect("2^31 elements in two factors", mi355_reverse_axes(src, dst, 65536, 32768, 1, 1, 1, nullptr), E, "2^31 elements or more");
    expect("INT_MAX in every dimension", mi355_reverse_axes(src, dst, INT_MAX, INT_MAX, INT_MAX, INT_MAX, 4, nullptr), E, "2^31 elements or more");
    expect("in place", mi355_reverse_axes(src, src, 2, 3, 4, 5, 4, nullptr), E, "overlap");
    expect("destination inside the source", mi355_reverse_axes(a, a + 4, 2, 3, 4, 5, 4, nullptr), E, "overlap");
    expect("source inside the destination", mi355_reverse_axes(a + 476, a, 2, 3, 4, 5, 4, nullptr), E, "overlap");
    expect("last byte shared", mi355_reverse_axes(a, a + 119, 2, 3, 4, 5, 1, nullptr), E, "overlap");
    expect("float32 at an odd address", mi355_reverse_axes(a + 1, dst, 2, 3, 4, 5, 4, nullptr), E, "not aligned to 4 bytes");
    // everything passes: the call ends at the device binding on a machine without a device
    const int rc = mi355_reverse_axes(a, a + 120, 2, 3, 4, 5, 1, nullptr);
    expect("touching, not overlapping (no device here)", rc, rc == MI355_OK ? MI355_OK : MI355_ERR_NO_DEVICE, nullptr);
    printf(failures ? "%d FAILURES\n" : "all refusals as expected\n", failures);
    return failures ? 1 : 0;
}
