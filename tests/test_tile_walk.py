"""The tile walk of the ENet kernels (csrc/bugseg_internal.h tile_walk) through its host-only debug entry
(bugseg_debug_tile_walk): ascending and descending walks visit the same tiles, each exactly once, per
XCD group in opposite order, and exactly the workgroups the ascending walk sends home get no tile."""
import pytest

from bugcar_image_segmentation_amd import _native as N

CASES = [(1, 8), (5, 8), (7, 8), (8, 8), (9, 8), (150, 8), (150, 64), (961, 256), (9600, 1024)]


@pytest.fixture(scope="module")
def walks(native_lib):
    return {(nt, g, rev): N.tile_walk(nt, g, rev) for nt, g in CASES for rev in (0, 1)}


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("ntiles,grid", CASES)
def test_every_tile_exactly_once(walks, ntiles, grid, rev):
    seq = walks[ntiles, grid, rev]
    assert len(seq) == grid
    flat = [t for wg in seq for t in wg]
    assert all(0 <= t < ntiles for t in flat)
    assert sorted(flat) == list(range(ntiles))


@pytest.mark.parametrize("ntiles,grid", CASES)
def test_ascending_walk_is_the_parents(walks, ntiles, grid):
    """rev = 0: workgroup b (group b % 8, slot b // 8) takes tiles grp * CH + slot, + grid / 8, ... while
    they stay inside the group's run and below ntiles."""
    ch, nslots = (ntiles + 7) // 8, grid // 8
    for b, wg in enumerate(walks[ntiles, grid, 0]):
        grp, slot = b % 8, b // 8
        want = [grp * ch + it for it in range(slot, ch, nslots) if grp * ch + it < ntiles]
        assert wg == want


@pytest.mark.parametrize("ntiles,grid", CASES)
def test_descending_walk_mirrors_each_group(walks, ntiles, grid):
    """Per XCD group the two directions cover the same run of tiles; step k of the descending walk is the
    run's k-th tile from its end, so every workgroup's sequence descends."""
    ch, nslots = (ntiles + 7) // 8, grid // 8
    up, down = walks[ntiles, grid, 0], walks[ntiles, grid, 1]
    for grp in range(8):
        members = range(grp, grid, 8)
        run_up = sorted(t for b in members for t in up[b])
        run_down = sorted(t for b in members for t in down[b])
        assert run_up == run_down
        assert run_up == list(range(grp * ch, grp * ch + len(run_up)))      # contiguous: the group's L2 run
        for b in members:
            slot = b // 8
            assert down[b] == [run_up[len(run_up) - 1 - it] for it in range(slot, len(run_up), nslots)]
            assert down[b] == sorted(down[b], reverse=True)
            assert len(down[b]) == len(up[b])


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("ntiles,grid", CASES)
def test_idle_workgroups_are_the_parents(walks, ntiles, grid, rev):
    """The parent's early return: workgroup b leaves when slot >= CH or grp * CH + slot >= ntiles. Exactly
    those workgroups get no tile, in either direction."""
    ch = (ntiles + 7) // 8
    for b, wg in enumerate(walks[ntiles, grid, rev]):
        grp, slot = b % 8, b // 8
        home = slot >= ch or grp * ch + slot >= ntiles
        assert (len(wg) == 0) == home


def test_bad_arguments_are_refused(native_lib):
    for nt, g, rev in [(0, 8, 0), (8, 0, 0), (8, 12, 0), (8, 8, 2)]:
        with pytest.raises(ValueError):
            N.tile_walk(nt, g, rev)
