"""CPU-side checks of the v1 forward-only path: the new entry points refuse invalid arguments with -22 before any HIP call (no GPU
is present here), the v2v rank definition the kernel computes agrees with a restatement of the reference script's loop
(v1/downstream/run_class_zero.py:389-404), and recall_at reproduces the reference fixture's R@k."""
import ctypes

import numpy as np
import pytest
import torch

import v1_downstream_synth as S
from tvts_amd import _lib
from tvts_amd.downstream import zero_shot as Z


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _buf(n=64):
    return ctypes.cast(ctypes.create_string_buffer(n), ctypes.c_void_p)


def test_new_entry_points_are_declared_with_their_reference_sites():
    protos = _lib.parse_header()
    for name in ("tvts_attn_fwd_first", "tvts_attn80_fwd_first", "tvts_patch_gather_tube_u8", "tvts_patch_gather_tube_cm",
                 "tvts_v2v_ranks"):
        assert name in protos, name
    src = open(_lib.HEADER_PATH).read()
    for site in ("video_encoder_zero.py:198-199", "model_dist_TVTS.py:131-141", "ssv2.py:61-63", "video_encoder_zero.py:91-96",
                 "run_class_zero.py:344-413"):
        assert site in src, site


def test_first_row_attention_refuses_bad_arguments(lib):
    for fn in (lib.tvts_attn_fwd_first, lib.tvts_attn80_fwd_first):
        assert fn(None, 192, 2, 1, 0, None, None, 64, None, None) == -22          # S = 0, no qkv, no kv_len
        assert fn(_buf(), 192, 2, 1, 0, None, _buf(), 64, None, None) == -22      # S = 0 with pointers
        assert fn(_buf(), 192, 0, 1, 4, None, _buf(), 64, None, None) == -22      # B = 0
        assert fn(_buf(), 191, 2, 1, 4, None, _buf(), 64, None, None) == -22      # ld % 8
        assert fn(None, 192, 2, 1, 4, None, _buf(), 64, None, None) == -22        # no qkv
        assert fn(_buf(), 192, 2, 1, 4, None, None, 64, None, None) == -22        # no out


def test_tube_gathers_refuse_bad_arguments(lib):
    m3, s3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.2, 0.2, 0.2)
    u8 = lambda H0, W0, img, patch, ldo, n=4, frames=_buf(), keep=_buf(): lib.tvts_patch_gather_tube_u8(  # noqa: E731
        frames, H0, W0, None, keep, 2, 3, 2, n, img, patch, m3, s3, _buf(), ldo, None)
    assert u8(40, 40, 32, 12, 3 * 2 * 144) == -22      # patch % 8 != 0
    assert u8(31, 40, 32, 16, 3 * 2 * 256) == -22      # H0 < img
    assert u8(40, 31, 32, 16, 3 * 2 * 256) == -22      # W0 < img
    assert u8(40, 40, 32, 16, 3 * 2 * 256 + 4) == -22  # ldo % 8
    assert u8(40, 40, 32, 16, 3 * 2 * 256 - 8) == -22  # ldo < row width
    assert u8(40, 40, 32, 16, 3 * 2 * 256, n=0) == -22
    assert u8(40, 40, 32, 16, 3 * 2 * 256, frames=None) == -22
    assert u8(40, 40, 40, 16, 3 * 2 * 256) == -22      # img % patch
    assert u8(40, 40, 0, 16, 3 * 2 * 256) == -22       # img <= 0
    cm = lambda img, patch, ldo, B=2, video=_buf(): lib.tvts_patch_gather_tube_cm(  # noqa: E731
        video, _buf(), B, 3, 2, 4, img, patch, _buf(), ldo, None)
    assert cm(32, 12, 3 * 2 * 144) == -22
    assert cm(40, 16, 3 * 2 * 256) == -22
    assert cm(32, 16, 3 * 2 * 256 - 8) == -22
    assert cm(32, 16, 3 * 2 * 256, B=0) == -22
    assert cm(0, 16, 3 * 2 * 256) == -22               # img <= 0 (0 % patch == 0 would pass the divisibility test)
    assert cm(-32, 16, 3 * 2 * 256) == -22
    assert cm(32, 16, 3 * 2 * 256, video=None) == -22
    # the 16-byte conditions of the shared frame (the bf16x8 store of every form, the f32x4 loads of the fp32 forms) and the NULL
    # pointers of tvts_patch_gather_tube; everything else about these calls is valid
    room = ctypes.create_string_buffer(96)
    at = lambda off: ctypes.c_void_p(((ctypes.addressof(room) + 15) & ~15) + off)  # noqa: E731
    assert lib.tvts_patch_gather_tube_u8(_buf(), 40, 40, None, _buf(), 2, 3, 2, 4, 32, 16, m3, s3, at(8), 3 * 2 * 256, None) == -22
    assert lib.tvts_patch_gather_tube_cm(at(0), _buf(), 2, 3, 2, 4, 32, 16, at(8), 3 * 2 * 256, None) == -22
    assert lib.tvts_patch_gather_tube_cm(at(4), _buf(), 2, 3, 2, 4, 32, 16, at(0), 3 * 2 * 256, None) == -22
    tube = lambda video=at(0), keep=_buf(), out=at(0), ldo=3 * 2 * 256: lib.tvts_patch_gather_tube(  # noqa: E731
        video, keep, 2, 3, 2, 4, 32, 16, out, ldo, None)
    assert tube(video=None) == -22 and tube(keep=None) == -22 and tube(out=None) == -22
    assert tube(video=at(4)) == -22 and tube(out=at(8)) == -22
    assert tube(ldo=3 * 2 * 256 + 4) == -22 and tube(ldo=3 * 2 * 256 - 8) == -22


def test_v2v_ranks_refuses_bad_arguments(lib):
    f = lambda ld, nq, q0, N, sims=_buf(), labels=_buf(), ranks=_buf(): lib.tvts_v2v_ranks(  # noqa: E731
        sims, ld, nq, q0, N, labels, ranks, None)
    assert f(4, 1, 0, 0) == -22        # N <= 0
    assert f(4, 1, 0, -3) == -22
    assert f(4, 0, 0, 4) == -22        # nq <= 0
    assert f(4, 3, 2, 4) == -22        # q0 + nq > N
    assert f(4, 1, -1, 4) == -22       # q0 < 0
    assert f(3, 1, 0, 4) == -22        # ld < N
    assert f(4, 1, 0, 4, sims=None) == -22
    assert f(4, 1, 0, 4, labels=None) == -22
    assert f(4, 1, 0, 4, ranks=None) == -22


def test_recall_at_reproduces_the_fixture(golden):
    f = golden("v1_downstream")
    assert Z.recall_at(f["v2v_ranks"]) == [float(v) for v in f["v2v_recall"]]
    assert Z.recall_at(torch.tensor([0.0, 4.0, 5.0, 9.0, 10.0, 1e20]), ks=(1, 5, 10)) == [100 / 6, 200 / 6, 400 / 6]
    # the fixture's ranks are what the restated loop gives on the regenerated features (the generator and this test share the seeds)
    feats, labels = S.v2v_data(int(f["v2v_seed"]))
    assert np.array_equal(labels.numpy(), f["v2v_labels"])
    assert np.array_equal(S.script_ranks(S.sim_matrix_np(feats), labels.numpy()), f["v2v_ranks"])
    assert int((labels == labels.max()).sum()) == 1  # one class with a single member


@pytest.mark.parametrize("seed", range(12))
def test_rank_definition_agrees_with_the_script_loop(seed):
    """Checks the DEFINITION, not the kernel: both sides are host restatements (tests/v1_downstream_synth.py), no product code runs
    here; the kernel is held to the same definition in tests/test_v1_infer_gpu.py::test_v2v_ranks_exact.
    `ranks < k` of the kernel's definition equals the script's hit among the first k of argsort(-scores) for every k <= 10, with
    fewer than ten videos included (there the script finds the query itself, at -1000, in the last position)."""
    g = torch.Generator().manual_seed(1000 + seed)
    for _ in range(25):
        N = int(torch.randint(2, 60, (1,), generator=g))
        classes = int(torch.randint(1, 8, (1,), generator=g))
        feats, labels = S.v2v_data(int(torch.randint(0, 1 << 30, (1,), generator=g)), N=N, D=16, classes=classes)
        s, lab = S.sim_matrix_np(feats), labels.numpy()
        same = lab[None, :] == lab[:, None]
        best = np.where(same, s, -np.inf).max(axis=1)
        assert not (~same & (s == best[:, None])).any()  # no tie between `best` and a different-label score
        mine, script = S.defined_ranks(s, lab), S.script_ranks(s, lab)
        for k in range(1, 11):
            assert np.array_equal(mine < k, script < k), (N, classes, k)
