"""wx_log_mel under the probes of tests/mel_probes.py (-m gpu): the impulse train (every tap in every
frame slot), the edge impulses (right padding 0 .. 201, chunks apart and back to back), the skip
boundary, every even bin tone, the edge bins, two-level tones, tilted noise and the chunk maxima, each
set within 4 x ref_err(set) of the fp64 evaluation on the CPU (ref_err: the reference's fp32 formula
against the same fp64, printed beside the kernel's figure), and NaN against zeros in everything a chunk
must not depend on.  One or two launches per test; no reference is computed on the GPU."""
import pytest
import torch

import mel_probes as mp

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
TRAIN_128_STARTS = (0, 39, 40, 159)


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _kernel(p):
    """The probe's call through wx_log_mel into a sentinel-filled output two frames wider than the
    longest chunk: what lies past a chunk's frames stays, the rest comes back per chunk."""
    from whisperx_amd import _lib

    frames = max(p.frames(b) for b in range(p.B))
    parent = torch.full((p.B, p.n_mels, frames + 2), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.log_mel(torch.from_numpy(p.wave).cuda(), p.first, p.length, p.pad, torch.from_numpy(p.filt.copy()).cuda(),
                 out=parent[:, :, 1:frames + 1])
    got = parent.cpu().numpy()
    outs = []
    for b in range(p.B):
        assert (got[b, :, 0] == SENTINEL).all() and (got[b, :, 1 + p.frames(b):] == SENTINEL).all(), (p.name, b)
        outs.append(got[b, :, 1:1 + p.frames(b)])
    return outs


@pytest.mark.parametrize("n_mels", [80, 128])
def test_impulse_train_every_tap_in_every_frame_slot(n_mels):
    st = mp.impulse_train(80) if n_mels == 80 else mp.impulse_train(128, TRAIN_128_STARTS)
    if n_mels == 80:
        assert st.pairs == 25408
    st.check(_kernel, "wx_log_mel")


@pytest.mark.parametrize("n_mels", [80, 128])
def test_edge_impulses_right_padding_0_to_201_apart_and_back_to_back(n_mels):
    mp.edge_impulses(n_mels).check(_kernel, "wx_log_mel")


@pytest.mark.parametrize("n_mels", [80, 128])
def test_skip_boundary_is_within_the_bound_and_bit_equal(n_mels, monkeypatch):
    st = mp.skip_boundary(n_mels)
    runs = {}
    for skip in (True, False):
        if skip:
            monkeypatch.delenv("WX_NO_MEL_SKIP", raising=False)
        else:
            monkeypatch.setenv("WX_NO_MEL_SKIP", "1")
        runs[skip] = _kernel(st.probes[0])
        st.check(lambda p: runs[skip], "skip on" if skip else "skip off")
    monkeypatch.delenv("WX_NO_MEL_SKIP")
    mp.check_bit_equal(st.probes[0], runs[True], runs[False], "skip on / off")


@pytest.mark.parametrize("n_mels", [80, 128])
def test_even_bin_tones_every_filterbank_entry(n_mels):
    st = mp.even_tones(n_mels)
    print(f"{st.name}: {st.entries} filterbank entries a decade above the floor, {100 * st.at_floor:.1f} % of the outputs at the floor")
    st.check(_kernel, "wx_log_mel")


@pytest.mark.parametrize("n_mels", [80, 128])
def test_edge_bins_through_moved_filterbank_columns(n_mels):
    mp.edge_bins(n_mels).check(_kernel, "wx_log_mel")


@pytest.mark.parametrize("n_mels", [80, 128])
def test_two_level_tones_and_tilted_noise(n_mels):
    mp.two_level_tones(n_mels).check(_kernel, "wx_log_mel")
    mp.tilted_noise(n_mels).check(_kernel, "wx_log_mel")


@pytest.mark.parametrize("n_mels", [80, 128])
def test_chunk_maxima_are_per_chunk_and_over_every_block(n_mels):
    mp.maxima(n_mels).check(_kernel, "wx_log_mel")


@pytest.mark.parametrize("n_mels", [80, 128])
def test_poison_outside_the_chunks_and_in_a_neighbour(n_mels):
    assert mp.check_poison_outside(_kernel, n_mels) > 0
    assert mp.check_poison_neighbour(_kernel, n_mels) > 0
