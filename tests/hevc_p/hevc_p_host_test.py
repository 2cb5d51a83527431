"""HEVC P pictures (hevc_inter: zero-motion skip / merge CTUs plus intra)
on the CPU encoder and the CPU pipeline, checked against the from-spec
decoder hevc_p_ref_decoder.DecoderP. No GPU.

Every chain test decodes the whole chain IDR, P, P... of a stripe and
compares the encoder's recon planes with the decoder's last picture
exactly. The CPU pipeline's debug dump holds stripe 0 only; the cases with
more than one stripe (QP sweep, mask, idr_frames) therefore go through
hevc_p_cases.check_recon_per_stripe_cpu, which encodes every stripe again
as a picture of its own, requires the same bytes, and compares that run's
recon, so every stripe, the 11-row partial one included, is compared
exactly. Every test that passes hevc_inter fails on a build without the
feature."""

import json
import pathlib
import shutil
import subprocess

import pytest

hipflux = pytest.importorskip("hipflux")
if not hipflux.native_available():
    pytest.skip("hipflux native module not built", allow_module_level=True)

from hipflux import _native
import pipeline_content as pc
import hevc_ref_decoder as hrd
import hevc_p_ref_decoder as prd
import hevc_p_cases as cases


def _checked(name):
    out, dump, _, w, h, sh, _ = cases.cpu_case(name)
    dec = cases.check_recon(out, dump, sh, stripes=[0])[0]
    return out, dec


# ---- 1. static content: all skip, tiny stripes, no parameter sets ----------

def test_static_is_all_skip_and_tiny():
    out, dec = _checked("static")
    assert [p[0] for p in dec.pictures] == [19, 1, 1]
    assert [p[1] for p in dec.pictures] == [0, 1, 2]
    for poc in (1, 2):
        assert cases.p_kinds(dec, poc) == ["skip"] * 10
    chain = cases.stripe_chain(out, 0)
    assert [c[3] for c in chain] == [True, False, False]
    assert set(cases.nal_types(chain[0][1])) >= cases.PARAMETER_SET_NALS
    for _, data, _, _ in chain[1:]:
        # per slice NAL: 6 start code + NAL header, <= 6 slice header, and
        # its skip + terminate bins (10 + 10 in the stripe) well inside 8
        # bytes; the whole stripe (two CTU rows, two slices) stays <= 32
        assert len(data) <= 32, len(data)
        types = cases.nal_types(data)
        assert types == [1, 1], types
        assert not set(types) & cases.PARAMETER_SET_NALS


# ---- 2. one changed block: exactly that CTU is coded -----------------------

@pytest.mark.parametrize("variant", ["grey", "colour"])
def test_patch_codes_one_ctu(variant):
    out, dec = _checked(f"patch-{variant}")
    kinds = cases.p_kinds(dec, 1)
    assert len(kinds) == 10
    # the 8x8 block lies in CTU column 1, row 1 -> address 6
    assert [i for i, k in enumerate(kinds) if k != "skip"] == [6], kinds


# ---- 3. half unchanged, half new: skip, then intra --------------------------

def test_half_and_half_mixes_inter_and_intra():
    out, dec = _checked("half")
    ctus = [c for c in dec.p_ctus if c["poc"] == 1]
    kinds = [c["kind"] for c in ctus]
    assert "intra" in kinds and ("skip" in kinds or "merge" in kinds), kinds
    for row in (0, 1):
        r = ctus[row * 5:row * 5 + 5]
        assert [c["kind"] for c in r[:3]] == ["skip"] * 3
        assert [c["kind"] for c in r[3:]] == ["intra"] * 2
        # first CTU of the slice: no left CTU; then left is skip
        assert [c["skip_ctx"] for c in r] == [0, 1, 1, 1, 0]
        # intra after skip: MPM candidate A is DC (left not intra)
        assert r[3]["cand_a"] == 1
        assert r[4]["cand_a"] == r[3]["mode"]


def test_kinds_and_cbf_luma_coverage():
    """Across this file's cases: every CTU kind, and cbf_luma both coded
    and inferred in merge CTUs."""
    decs = [_checked(n)[1] for n in ("static", "patch-grey", "patch-colour",
                                     "half", "qp26")]
    kinds = {c["kind"] for d in decs for c in d.p_ctus if c["poc"] > 0}
    assert kinds == {"skip", "merge", "intra"}, kinds
    merge_coded = {c["cbf_luma_coded"] for d in decs for c in d.p_ctus
                   if c["kind"] == "merge"}
    assert merge_coded == {True, False}, merge_coded


# ---- 4. QP sweep at an odd size --------------------------------------------

@pytest.mark.parametrize("qp", [0, 26, 30, 44, 51])
def test_qp_sweep_odd_size(qp):
    """161x75, stripe 32: odd sizes, a partial last stripe, padding columns
    predicted from the unclamped reference."""
    out, dump, _, w, h, sh, _ = cases.cpu_case(f"qp{qp}")
    dec = cases.check_recon(out, dump, sh, stripes=[0])[0]
    assert [p[1] for p in dec.pictures] == [0, 1, 2]
    # every stripe's recon, the 11-row partial last one included
    decs = cases.check_recon_per_stripe_cpu(f"qp{qp}")
    assert sorted(decs) == [0, 32, 64]
    for y0, d in decs.items():
        assert [p[1] for p in d.pictures] == [0, 1, 2]


# ---- 5. slice segments that start mid-row ----------------------------------

def test_segments_start_mid_row():
    out, dec = _checked("half-spr3")
    chain = cases.stripe_chain(out, 0)
    assert cases.nal_types(chain[1][1]) == [1] * 6   # 2 rows x 3 segments
    ctus = [c for c in dec.p_ctus if c["poc"] == 1]
    for row in (0, 1):
        r = ctus[row * 5:row * 5 + 5]
        # segments [0,1] [2,3] [4]: a segment's first CTU has no left CTU
        assert [c["skip_ctx"] for c in r] == [0, 1, 0, 1, 0]
        assert r[4]["kind"] == "intra" and r[4]["cand_a"] == 1


# ---- 6. POC counts a stripe's own coded pictures ---------------------------

def test_mask_poc_counts_coded_pictures():
    out, dump, _, w, h, sh, _ = cases.cpu_case("mask")
    cases.check_recon(out, dump, sh, stripes=[0])
    assert sorted(cases.check_recon_per_stripe_cpu("mask")) == [0, 16, 32]
    coded = {0: [0, 2, 3], 16: [0, 1, 3], 32: [0, 2, 3]}
    for y0, frames in coded.items():
        chain = cases.stripe_chain(out, y0)
        assert [c[0] for c in chain] == frames
        assert [c[3] for c in chain] == [True, False, False]
        dec, pics = cases.decode_chain(out, y0)
        assert [(p[0], p[1], p[2]) for p in dec.pictures] == \
            [(19, 0, 0), (1, 1, 1), (1, 2, 2)]


def test_idr_frames_restart_the_chain():
    out, dump, _, w, h, sh, _ = cases.cpu_case("idr")
    cases.check_recon(out, dump, sh, stripes=[0])
    assert sorted(cases.check_recon_per_stripe_cpu("idr")) == [0, 16, 32]
    for y0 in (0, 16, 32):
        chain = cases.stripe_chain(out, y0)
        assert [c[3] for c in chain] == [True, False, True, False]
        assert set(cases.nal_types(chain[2][1])) >= cases.PARAMETER_SET_NALS
        assert not set(cases.nal_types(chain[3][1])) & \
            cases.PARAMETER_SET_NALS
        dec, _ = cases.decode_chain(out, y0)
        assert [(p[0], p[1]) for p in dec.pictures] == \
            [(19, 0), (1, 1), (19, 0), (1, 1)]


def test_poc_wraps_at_256():
    out, dec = _checked("wrap")
    assert len(dec.pictures) == 260
    assert [p[1] for p in dec.pictures] == list(range(260))
    assert [p[2] for p in dec.pictures[254:258]] == [254, 255, 0, 1]


def test_missing_reference_raises():
    """The decoder does not invent a reference: a chain with a P picture
    cut out fails at the next P picture."""
    out, _ = _checked("static")
    chain = cases.stripe_chain(out, 0)
    with pytest.raises(ValueError, match="no reference picture"):
        prd.DecoderP().decode(chain[0][1] + chain[2][1])


# ---- 7. the flag is neutral when it cannot act ------------------------------

def test_flag_off_and_fullcolor_are_unchanged():
    fr = list(pc.frames_for(96, 48, 3))
    args = ("cpu", fr, 96, 48, 26, 16, 2)
    plain = _native._pipeline_encode(*args)
    off = _native._pipeline_encode(*args, hevc_inter=False)
    assert pc.per_frame(off) == pc.per_frame(plain)
    assert all(key for f in off for _, _, _, key in f)
    fc = _native._pipeline_encode(*args, fullcolor=True)
    fc_inter = _native._pipeline_encode(*args, fullcolor=True,
                                        hevc_inter=True)
    assert pc.per_frame(fc_inter) == pc.per_frame(fc)
    assert all(key for f in fc_inter for _, _, _, key in f)
    on = _native._pipeline_encode(*args, hevc_inter=True)
    assert pc.per_frame(on) != pc.per_frame(plain)


# ---- 8. context tables ------------------------------------------------------

def test_init_tables_match_the_decoder():
    for init_type, table in ((0, hrd.INIT), (1, prd.INIT1)):
        got = list(_native._hevc_init_values(init_type))
        assert len(got) == 129
        assert all(0 <= v <= 255 for v in got)
        want = []
        for name in prd.BANK_ORDER:
            # initType 0 has no P-only elements; the bank pads with 154
            want += table.get(name, [154] * len(prd.INIT1[name]))
        assert got == want
    assert prd.INIT1["last_x"] == prd.INIT1["last_y"]
    assert all(0 <= v <= 255 for vals in prd.INIT1.values() for v in vals)
    assert sum(len(v) for v in prd.INIT1.values()) == 129


# ---- 9. engine: delta stripes, and key stripes on request -------------------

def test_engine_emits_delta_then_key_stripes_on_request():
    cases.engine_delta_then_key(use_cpu=True, pipeline="cpu-hevc")


# ---- 10. web client: delta stripes keep the row's codec ----------------------

JS_HARNESS = """
const fs = require("fs");
const src = fs.readFileSync(process.argv[2], "utf8");
const a = src.match(/\\/\\* hevcCodecString:begin[\\s\\S]*?hevcCodecString:end \\*\\//);
const b = src.match(/\\/\\* hevcStripeCodec:begin[\\s\\S]*?hevcStripeCodec:end \\*\\//);
if (!a || !b) { console.error("marker block not found"); process.exit(2); }
const f = new Function(a[0] + b[0] + "; return hevcStripeCodec;")();
const [keyHex, deltaHex] = process.argv.slice(3);
const bytes = (hex) => Uint8Array.from(Buffer.from(hex, "hex"));
const main = f(true, bytes(keyHex), null);
process.stdout.write(JSON.stringify([
  main,
  f(false, bytes(deltaHex), main),
  f(false, bytes(deltaHex), "hev1.4.10.L123.BE.8"),
  f(false, bytes(deltaHex), null),
]));
"""


@pytest.mark.skipif(shutil.which("node") is None, reason="node not available")
def test_js_delta_stripe_keeps_row_codec(tmp_path):
    web = pathlib.Path(__file__).resolve().parents[2] / "selkies_amd" / "web"
    out, _ = _checked("static")
    chain = cases.stripe_chain(out, 0)
    key, delta = chain[0][1], chain[1][1]
    # a delta stripe starts with a TRAIL_R slice; byte 10 is slice data,
    # which hevcCodecString would misread as a profile
    assert (delta[4] >> 1) & 0x3F == 1
    harness = tmp_path / "run.js"
    harness.write_text(JS_HARNESS)
    r = subprocess.run(["node", str(harness), str(web / "selkies-client.js"),
                        key[:64].hex(), delta[:64].hex()],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout) == ["hev1.1.6.L123.B0", "hev1.1.6.L123.B0",
                                    "hev1.4.10.L123.BE.8", None]


# ---- 11. the server-side setting ---------------------------------------------

def test_setting_is_off_by_default_and_structural():
    from selkies_amd.settings import load_settings
    from selkies_amd.streaming import StreamingService
    assert load_settings([], env={}).hevc_inter is False
    assert load_settings(["--hevc-inter", "true"], env={}).hevc_inter is True
    assert "hevc_inter" in StreamingService.STRUCTURAL
    assert hipflux.CaptureSettings().hevc_inter is False
