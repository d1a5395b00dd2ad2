"""The plane Hill sweep pipelined a whole tile ahead.  k_sweep_light_plane consumes at the top of a pass what
it requested a pass earlier -- the streams and the four gathered du values of its tile -- through a connectivity requested two
passes earlier, and a clamped element index stands in for a tile past the end.  None of that may be seen in a result: every case
runs with PLFX_PLANE_COLS=1 (the pipelined kernel) and =0 (k_sweep_light<1>, untouched) in one process and compares the full list
of tests/test_gpu_plane_cols.py with np.array_equal -- u, f, du, sig, eps, epl, sgl, egl, epgl, niter, the PCG iterations,
res_sig, res_depl, fyn, max_steps and the expanded tangents -- and asserts through plane_info() that plane sweeps ran (on_off of
that file, whose helpers these cases reuse).

The cases are the edges of the pipeline, with the grid capped by PLFX_SWEEP_BLOCKS:
  1 block, 225 elements (15 x 15): one pass, both look-aheads wholly past the end;
  1 block, 256 and 512 elements (16 x 16, 32 x 16): the tile after the last one starts exactly at nel, no partial tile;
  1 block, 625 elements (25 x 25): three passes, partial last tile;
  2 and 3 blocks, 1160 elements (40 x 29, five tiles): threads with 3 and 2, and with 2, 2 and 1 passes;
all on the mixed model (Hill | elastic | softer Hill: lanes that drop out of the arithmetic beside lanes that do not); the bench
tension model with the soft inclusion at 128 x 128 in five blocks (13 and 12 passes): elements go to the corrector list, sweeps
run armed and unarmed, load steps end at nit = 15, so full-form old tangents (the 21 loads of the cold branch, beside the
prefetch in flight) are met; the all-plastic model in one block, stopped and resumed; and, with no cap from the environment, the
bench tension model at 416 x 320 (520 tiles), more tiles than the blocks the device holds at once, which is the sweep's grid."""
import numpy as np
import pytest

from test_gpu_dead_stores import EPS, inclusion, solved
from test_gpu_end_of_step import plastic_model
from test_gpu_plane_cols import ON, SWITCH, arrays, assert_premise, assert_same, on_off
from test_gpu_sweep_prefetch import mixed_model

pytestmark = pytest.mark.gpu

TILE = 256   # BLOCK of plfx_kernels.hpp: elements per tile


def passes(nel, blocks):
    """tile-loop passes of the threads of each block: tiles b, b + blocks, ... below ceil(nel / TILE)"""
    tiles = (nel + TILE - 1) // TILE
    return [len(range(b, tiles, blocks)) for b in range(blocks)]


@pytest.mark.parametrize('blocks,nx,ny,want,corrector', [
    (1, 15, 15, [1], True),            # one pass; tiles t + nb and t + 2 nb lie wholly past the end
    (1, 16, 16, [1], False),           # exactly one tile: the next one starts at nel
    (1, 32, 16, [2], False),           # exactly two
    (1, 25, 25, [3], True),            # three passes, the last tile partial (113 elements)
    (2, 40, 29, [3, 2], True),         # five tiles, the last partial (136 elements)
    (3, 40, 29, [2, 2, 1], True)])
def test_mixed_model_pipeline_edges(monkeypatch, blocks, nx, ny, want, corrector):
    assert passes(nx * ny, blocks) == want
    a, b, fe = on_off(monkeypatch, lambda: mixed_model(nx, ny, EPS), 2, PLFX_SWEEP_BLOCKS=str(blocks))
    hit = int(np.sum(a['max_steps'].ravel() >= 49))
    print('%d x %d in %d block(s), passes %s: plane_info on %s off %s, sweeps / tangents rewritten %s, load steps %d, niter %s, '
          'elements through the corrector %d' % (nx, ny, blocks, want, a['plane'], b['plane'], tuple(a['sweeps']), int(a['nsteps']),
                                                 list(a['niter']), hit))
    assert fe.Nel == nx * ny and a['plane'][1] > 0
    assert np.max(a['niter']) >= 2 and np.max(np.abs(a['epl'])) > 0.
    mat = np.asarray(fe._mat_id)
    assert np.sum(mat == 1) > 0 and not np.any(a['fyn'][mat == 1])    # the elastic section: lanes without a return mapping
    assert a['dead'][0] > 0 and a['dead'][1] > 0                       # armed sweeps rewrote tangents
    if corrector:   # (the meshes of tests/test_gpu_plane_cols.py, where this is known to hold)
        assert hit > 0


def test_inclusion_many_passes_corrector_and_iteration_limit(monkeypatch):
    nx = ny = 128
    blocks = 5
    assert sorted(set(passes(nx * ny, blocks))) == [12, 13]
    a, b, fe = on_off(monkeypatch, lambda: inclusion(nx, ny), 50, 12, PLFX_SWEEP_BLOCKS=str(blocks))
    at_limit = int(np.sum(a['niter'] == 15))
    print('inclusion %d x %d in %d blocks: plane_info %s, dead_store_info %s, sweeps / tangents rewritten %s, niter %s'
          % (nx, ny, blocks, a['plane'], tuple(a['dead']), tuple(a['sweeps']), list(a['niter'])))
    assert int(a['nsteps']) == 12 and np.max(np.abs(a['epl'])) > 0.
    assert np.sum(a['max_steps'].ravel() >= 49) > 0            # the corrector list was not empty
    assert at_limit >= 2 and a['niter'][-1] == 15              # averaged full-form tangents written, and met again as old tangents
    assert a['dead'][0] > 0 and a['sweeps'][0] - a['dead'][0] == at_limit    # armed sweeps, and the unarmed one of each such step


def test_more_tiles_than_resident_blocks(monkeypatch):
    """The sweep's grid is at most the blocks the device holds at once (two per CU: 512 on the 256 CUs of an MI355X).  The bench
    tension model at 416 x 320 has 520 tiles: without any cap from the environment, eight blocks take a second pass there."""
    from test_gpu_pred_start import tension
    nx, ny, steps = 416, 320, 8
    assert (nx * ny) // TILE == 520
    a, b, fe = on_off(monkeypatch, lambda: tension(nx, ny), 50, steps)
    print('%d elements: plane_info %s, dead_store_info %s, sweeps / tangents rewritten %s, niter %s'
          % (fe.Nel, a['plane'], tuple(a['dead']), tuple(a['sweeps']), list(a['niter'])))
    assert fe.Nel == nx * ny and int(a['nsteps']) == steps
    assert a['plane'][1] > 0 and a['dead'][1] >= fe.Nel and np.max(np.abs(a['epl'])) > 0.    # a sweep that rewrote every tangent


def test_all_plastic_one_block_stopped_and_resumed(monkeypatch):
    N, STOP = 40, 12
    monkeypatch.setenv('PLFX_SWEEP_BLOCKS', '1')
    runs = []
    for switch in ('1', '0'):
        monkeypatch.setenv('PLFX_PLANE_COLS', switch)
        fe = solved(plastic_model(), N, STOP)
        assert fe.nsteps == STOP and passes(fe.Nel, 1) == [3]
        mid = arrays(fe)
        first = list(fe.niter)
        solved(fe, N - STOP)
        runs.append((mid, arrays(fe), first + list(fe.niter)))
    (mid_a, a, nit_a), (mid_b, b, nit_b) = runs
    print('one block, stopped after %d load steps and resumed: plane_info at the stop %s at the end %s, niter %s'
          % (STOP, mid_a['plane'], a['plane'], nit_a))
    assert nit_a == nit_b and b['plane'] == (False, 0, 0, SWITCH)
    assert mid_a['plane'][0] and mid_a['plane'][1] == mid_a['sweeps'][0] > 0
    assert a['plane'][0] and a['plane'][3] == ON and a['plane'][1] == a['sweeps'][0] > mid_a['plane'][1]
    assert_premise(mid_b, fe)
    assert_premise(b, fe)
    assert_same(mid_a, mid_b)
    assert_same(a, b)
    assert not np.array_equal(mid_a['sig'], a['sig'])
