"""The tile tables of the sliding window off the cube and off step 0.5, checked without a device against the oracle's restatement
of nnU-Net's _compute_steps_for_sliding_window (oracle/tiler_ref.py), through the library's own entry points: mi355_compute_steps
and the dry run mi355_stage0_plan, which runs the make_geom a real window runs.

nnU-Net forms ``patch * step`` from the Python float, a double.  The step therefore crosses the C ABI as a double: carried as a
float32 it lands on the other side of the ceil for steps float32 does not hold exactly (0.3, 0.6, 0.7, 0.9) whenever image - patch
is a multiple of patch * step."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import pytest

from oracle import tiler_ref

STEPS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.25, 0.75, 1.0)
PATCHES = (32, 48, 64, 80, 96, 112, 128, 160, 192)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


def test_tile_tables_one_axis(ops):
    """Every step of STEPS x every patch of PATCHES x every image extent from patch to 4 * patch: the library's step table equals
    the oracle's, entry by entry.

    With the step carried as a float32 (the C ABI before this test) the built library disagreed on exactly these 23 rows, as
    (step, patch, image, tiles of the oracle, tiles of the library) - the first of them a BraTS in-plane extent, 240, under a
    96 patch:
        (0.3,  48, 120,  7,  6) (0.3,  48, 192, 12, 11) (0.3,  96, 240,  7,  6) (0.3,  96, 384, 12, 11)
        (0.3, 192, 480,  7,  6) (0.3, 192, 768, 12, 11)
        (0.6,  48, 192,  7,  6) (0.6,  96, 384,  7,  6) (0.6, 192, 768,  7,  6)
        (0.7,  80, 136,  2,  3) (0.7,  80, 192,  3,  4) (0.7,  80, 248,  4,  5) (0.7,  80, 304,  5,  6)
        (0.7, 160, 272,  2,  3) (0.7, 160, 384,  3,  4) (0.7, 160, 496,  4,  5) (0.7, 160, 608,  5,  6)
        (0.9,  80, 152,  2,  3) (0.9,  80, 224,  3,  4) (0.9,  80, 296,  4,  5)
        (0.9, 160, 304,  2,  3) (0.9, 160, 448,  3,  4) (0.9, 160, 592,  4,  5)"""
    bad = []
    for step in STEPS:
        for patch in PATCHES:
            for image in range(patch, 4 * patch + 1):
                want = tiler_ref.compute_steps_for_sliding_window((patch,), (image,), step)[0]
                got = ops.compute_steps(patch, image, step)
                if got != want:
                    bad.append((step, patch, image, len(want), len(got)))
    print(f"one-axis tile tables: {len(bad)} rows differ from the oracle: {bad}")
    assert bad == []


def test_tile_tables_any_step_a_double_holds(ops):
    """Seeded random steps in (0, 1] with all 53 bits in use, and the steps whose patch * step divides image - patch exactly or
    misses it by one ulp: the same arithmetic in the same precision lands on the same side of the ceil."""
    import numpy as np
    rs = np.random.RandomState(7)
    cases = [(float(rs.uniform(0.05, 1.0)), int(rs.choice(PATCHES)), None) for _ in range(3000)]
    for patch in PATCHES:
        for k in range(1, 9):   # image - patch = k targets: step = (image - patch) / (k * patch), and its two neighbours
            for image in (patch + 8 * k, patch + 13 * k):
                step = (image - patch) / (k * patch)
                cases += [(s, patch, image) for s in (step, np.nextafter(step, 0.0), np.nextafter(step, 2.0)) if 0.0 < s <= 1.0]
    for step, patch, image in cases:
        image = int(rs.randint(patch, 4 * patch + 1)) if image is None else image
        assert ops.compute_steps(patch, image, float(step)) == tiler_ref.compute_steps_for_sliding_window((patch,), (image,), float(step))[0], \
            (step, patch, image)


# non-cubic patches; volumes with a different odd excess on each axis, one below its patch (padded), one a float32 row of the table above
GRIDS = [((32, 48, 64), (41, 100, 75)), ((64, 32, 48), (75, 41, 100)), ((48, 64, 32), (120, 59, 97)), ((96, 48, 80), (240, 120, 136)),
         ((32, 48, 64), (29, 193, 64)), ((48, 96, 160), (192, 384, 304))]
STEPS_3D = (0.25, 0.3, 0.5, 0.75, 1.0)
MIRRORS = [m for k in range(4) for m in itertools.combinations(range(3), k)]


def _oracle_steps(patch, volume, step):
    padded = tuple(max(v, p) for v, p in zip(volume, patch))
    return padded, tiler_ref.compute_steps_for_sliding_window(patch, padded, step)


@pytest.mark.parametrize("step", STEPS_3D)
@pytest.mark.parametrize("patch, volume", GRIDS)
def test_tile_tables_three_axes(ops, patch, volume, step):
    """n_tiles and every sample's origin of mi355_stage0_plan, for every subset of mirror axes: tiles in the oracle's order (z
    outermost), a mirrored origin Zp - P - org on each flipped axis and on no other."""
    padded, steps = _oracle_steps(patch, volume, step)
    tiles = list(itertools.product(*steps))
    for axes in MIRRORS:
        p = ops.stage0_plan(volume, patch, step, axes, 2)
        assert p["padded"] == padded and p["n_tiles"] == len(tiles) and p["n_mirrors"] == 2 ** len(axes)
        assert p["shared"] == (len(tiles) > 1)
        if not p["shared"]:
            continue
        assert len(p["samples"]) == len(tiles) * p["n_mirrors"]
        seen = {}
        for s in p["samples"]:
            org = tiles[s["tile"]]
            assert set(s["mirror"]) <= set(axes)
            assert s["origin"] == tuple(padded[a] - patch[a] - org[a] if a in s["mirror"] else org[a] for a in range(3)), (axes, s)
            seen.setdefault(s["tile"], set()).add(s["mirror"])
        assert sorted(seen) == list(range(len(tiles))) and all(len(v) == p["n_mirrors"] for v in seen.values())


@pytest.mark.parametrize("step", STEPS_3D)
@pytest.mark.parametrize("patch, volume", GRIDS)
def test_tiles_of_shape_equals_the_library(ops, amd, patch, volume, step):
    """parallel.tiles_of_shape sizes the work of a rank: it must count the tiles the library produces."""
    assert amd.parallel.tiles_of_shape(volume, patch, step) == ops.stage0_plan(volume, patch, step, (), 2)["n_tiles"]


def test_tiles_of_shape_one_axis_scan(ops, amd):
    """... and over the one-axis scan, where the float32 step used to disagree with it."""
    for step in STEPS:
        for patch in PATCHES:
            for image in range(patch, 4 * patch + 1, 8):
                assert amd.parallel.tiles_of_shape((image, patch, patch), (patch, patch, patch), step) == len(ops.compute_steps(patch, image, step))


_SIZEOF_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "mi355_nnunet.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mi355_sw_opts), offsetof(mi355_sw_opts, patch), offsetof(mi355_sw_opts, step_size),
           offsetof(mi355_sw_opts, use_gaussian), offsetof(mi355_sw_opts, mirror_axes), offsetof(mi355_sw_opts, batch_tiles));
    return 0;
}
"""


def test_sw_opts_layout_matches_the_header(amd, tmp_path):
    """The double step puts 4 bytes of padding behind patch[3]: ctypes must lay mi355_sw_opts out as the C compiler lays out the
    header's struct - size and the offset of every field the predictor sets."""
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if subprocess.run(
        ["sh", "-c", f"command -v {c}"], capture_output=True).returncode == 0), None)
    assert cc, "no C compiler to lay the header's struct out"
    src, exe = tmp_path / "sizeof.c", tmp_path / "sizeof"
    src.write_text(_SIZEOF_C)
    r = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    S = amd._lib.SwOpts
    mine = [C.sizeof(S)] + [getattr(S, f).offset for f in ("patch", "step_size", "use_gaussian", "mirror_axes", "batch_tiles")]
    print(f"mi355_sw_opts (size, offsets): header {r.stdout.split()}, ctypes {mine}")
    assert [int(v) for v in r.stdout.split()] == mine
    assert mine[:3] == [40, 0, 16] and S.step_size.size == 8
    assert dict(S._fields_)["step_size"] is C.c_double


def test_step_crosses_the_abi_as_a_double(amd):
    lib = amd._lib.load()
    assert lib.mi355_compute_steps.argtypes[2] is C.c_double
    for fn in (lib.mi355_stage0_plan, lib.mi355_stage0_merge_plan, lib.mi355_skip_share_plan, lib.mi355_stage0_view_plan,
               lib.mi355_level1_share_plan):
        assert fn.argtypes[4] is C.c_double
