"""HEVC P pictures on the HIP pipeline (k_hevc_rows_p / k_hevc_cabac_p).

Each test runs a case of hevc_p_cases through the HIP pipeline and asserts
(a) its bytes equal the CPU pipeline's, per frame and stripe, and (b) its
debug-dump recon planes equal the from-spec decoder's last picture of the
HIP pipeline's own chain, for every stripe of the frame."""

import pytest

hipflux = pytest.importorskip("hipflux")
if not hipflux.native_available():
    pytest.skip("hipflux native module not built", allow_module_level=True)

import pipeline_content as pc
import hevc_p_cases as cases

pytestmark = pytest.mark.gpu


def _check(name, depth=1, **env):
    out, dump, cpu_out, sh = cases.gpu_run(name, depth, **env)
    got, want = pc.per_frame(out), pc.per_frame(cpu_out)
    assert len(got) == len(want)
    for i, (g, c) in enumerate(zip(got, want)):
        assert [y for y, _ in g] == [y for y, _ in c], f"frame {i} stripes"
        for (y, gb), (_, cb) in zip(g, c):
            assert gb == cb, f"frame {i} stripe at {y}: GPU bytes != CPU"
    keys = [[k for *_, k in f] for f in out]
    assert keys == [[k for *_, k in f] for f in cpu_out]
    decs = cases.check_recon(out, dump, sh)
    return out, decs


def test_static():
    out, decs = _check("static")
    assert cases.p_kinds(decs[0]) == ["skip"] * 20
    assert not any(k for f in out[1:] for *_, k in f)


@pytest.mark.parametrize("variant", ["grey", "colour"])
def test_patch(variant):
    _, decs = _check(f"patch-{variant}")
    kinds = cases.p_kinds(decs[0], 1)
    assert [i for i, k in enumerate(kinds) if k != "skip"] == [6]
    assert kinds[6] == "merge"


def test_half_and_half():
    _, decs = _check("half")
    assert set(cases.p_kinds(decs[0])) == {"skip", "intra"}


def test_half_and_half_host_entropy():
    """Rows kernel + host entropy coder: a failure here but not in the
    kernel-CABAC tests, or the reverse, names the kernel at fault."""
    _check("half", HIPFLUX_CPU_HEVC_ENTROPY=1)
    _check("patch-grey", HIPFLUX_CPU_HEVC_ENTROPY=1)


@pytest.mark.parametrize("qp", [0, 26, 30, 44, 51])
def test_qp_sweep_odd_size(qp):
    _check(f"qp{qp}")


def test_segments_start_mid_row():
    _check("half-spr3")


def test_mask_depth_1_and_2():
    out1, _ = _check("mask", depth=1)
    out2, _ = _check("mask", depth=2)
    assert pc.per_frame(out1) == pc.per_frame(out2)


def test_idr_frames():
    out, _ = _check("idr")
    assert [[k for *_, k in f] for f in out] == \
        [[True] * 3, [False] * 3, [True] * 3, [False] * 3]


def test_poc_wrap():
    _, decs = _check("wrap")
    assert [p[2] for p in decs[0].pictures[254:258]] == [254, 255, 0, 1]


def test_engine_emits_delta_then_key_stripes_on_request():
    cases.engine_delta_then_key(use_cpu=False, pipeline="hip-hevc")
