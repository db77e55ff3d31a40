"""The skewed tile order of the colour-gated fp32 kernel (ideal-nerf_amd/csrc/tile_order.h), checked exhaustively on the host:
the header is compiled with gcc into a stand-alone program that walks the order exactly as the kernel's loop does."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-nerf_amd", "csrc")
GRIDS = (1, 2, 3, 255, 256, 304)

# One line per (G, ntiles, c): "G ntiles c : tile/next tile/next ..." -- the tiles workgroup c renders, each with the tile its
# prefetch asked for, the loop being the kernel's own: start at c, stop at the first tile >= ntiles.  After the stop the walk
# goes on for three more rounds and prints those tiles behind a '|' (none of them may be in range).  A last line per G gives
# the closed form for the first rounds, "G : r c tile ...", and the step.
PROGRAM = r"""
#include <stdio.h>
#include "tile_order.h"
int main(void) {
    static const int grids[] = {%s};
    for (unsigned g = 0; g < sizeof grids / sizeof *grids; ++g) {
        const int G = grids[g], step = tile_order_step(G);
        for (long ntiles = 0; ntiles <= 3L * G + 2; ++ntiles)
            for (int c = 0; c < G; ++c) {
                long base = 0, next;
                int off = c;
                printf("%%d %%ld %%d :", G, ntiles, c);
                for (long tile = c; tile < ntiles; tile = next) {
                    next = tile_order_next(&base, &off, G, step);
                    printf(" %%ld/%%ld", tile, next);
                }
                printf(" |");
                for (int k = 0; k < 3; ++k) printf(" %%ld", tile_order_next(&base, &off, G, step));
                printf("\n");
            }
        printf("closed %%d %%d %%d :", G, step, IDN_TILE_SKEW);
        for (long r = 0; r < 5; ++r)
            for (int c = 0; c < G; ++c) printf(" %%ld", tile_order_tile(r, c, G));
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_order")
    prog, exe = d / "walk.c", d / "walk"
    prog.write_text(PROGRAM % ", ".join(map(str, GRIDS)))
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-I", CSRC, str(prog), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    per_case, closed = {}, {}
    for line in out.splitlines():
        head, tail = line.split(" :")
        if head.startswith("closed"):
            _, G, step, skew = head.split()
            closed[int(G)] = (int(step), int(skew), [int(x) for x in tail.split()])
            continue
        G, ntiles, c = map(int, head.split())
        run, after = tail.split("|")
        pairs = [tuple(map(int, p.split("/"))) for p in run.split()]
        per_case.setdefault((G, ntiles), {})[c] = (pairs, [int(x) for x in after.split()])
    return per_case, closed


def test_every_case_ran(walks):
    per_case, closed = walks
    assert sorted(closed) == sorted(GRIDS)
    assert len(per_case) == sum(3 * G + 3 for G in GRIDS)
    for (G, _), by_c in per_case.items():
        assert sorted(by_c) == list(range(G))


def test_the_skew_is_an_odd_stride_coprime_to_the_grid(walks):
    _, closed = walks
    for G, (step, skew, _) in closed.items():
        assert skew % 2 == 1 and step == skew % G and 0 <= step < max(G, 1)
    import math
    assert math.gcd(closed[256][1], 256) == 1 and math.gcd(closed[304][1], 304) == 1


def test_every_tile_exactly_once(walks):
    per_case, _ = walks
    for (G, ntiles), by_c in per_case.items():
        tiles = sorted(t for pairs, _ in by_c.values() for t, _ in pairs)
        assert tiles == list(range(ntiles)), (G, ntiles)


def test_nothing_in_range_after_the_first_out_of_range_tile(walks):
    """The loop stops a workgroup at its first tile >= ntiles; the tiles it would have had in later rounds are out of range too."""
    per_case, _ = walks
    for (G, ntiles), by_c in per_case.items():
        for c, (pairs, after) in by_c.items():
            stop = pairs[-1][1] if pairs else c
            assert stop >= ntiles, (G, ntiles, c)
            assert all(t >= ntiles for t in after), (G, ntiles, c, after)


def test_prefetched_tile_is_the_next_tile_rendered(walks):
    per_case, _ = walks
    for (G, ntiles), by_c in per_case.items():
        for c, (pairs, _) in by_c.items():
            for (_, nxt), (tile, _) in zip(pairs, pairs[1:]):
                assert nxt == tile, (G, ntiles, c)
            if pairs:
                assert pairs[0][0] == c and pairs[-1][1] >= ntiles   # round 0 is the identity; the last prefetch is the clamped one


def test_walk_is_the_closed_form(walks):
    """tile(r, c) = r G + ((c + r K) mod G): the incremental walk the kernel uses against the definition, round by round."""
    per_case, closed = walks
    for G, (_, skew, flat) in closed.items():
        for r in range(5):
            for c in range(G):
                assert flat[r * G + c] == r * G + (c + r * skew) % G
        by_c = per_case[(G, 3 * G + 2)]
        for c, (pairs, after) in by_c.items():
            seq = ([t for t, _ in pairs] + [pairs[-1][1]] + after)[:5]
            assert len(seq) == 5 and seq == [flat[r * G + c] for r in range(len(seq))], (G, c)
