"""The conv dispatch plan (csrc/kernels_conv.hip: conv_plan), asked through the host-only export sr3_conv_plan — no GPU.

tests/conv_plans.json is the table of plans of a fixed list of conv shapes: every conv of the UNet configurations the
other tests and the benchmark run (with fused statistics offered, as the engine offers them), and the single-conv rows of
test_gpu_conv_gates.py and test_gpu_ops.py (without, as sr3_op_conv2d runs them), each in all three precisions with every
environment switch unset. It was recorded from the launches of the library BEFORE the plan existed (the launch code
with its kernel launches replaced by a recorder) and the library must reproduce it exactly: a change of a gate, a
threshold or a tile choice shows up here as a diff of that file.

    python tests/test_conv_plan_host.py [path]      writes the table of the library in this tree (default: the file)
"""
import json
import os
import sys

import pytest

from conftest import pkg

import test_gpu_config_sweep as sweep
import test_gpu_conv_gates as gates
import test_gpu_ops as ops

engine = pkg("engine")
synth = pkg("synth")

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_plans.json")
SWITCHES = ("SR3_NO_HALO", "SR3_HALO_SPLITS", "SR3_NO_INPLACE_SPLIT", "SR3_NO_WINOGRAD")   # (SR3_NO_GRAPH: not a conv switch)
PRECISIONS = ("f32", "f16x3", "f16f8")
CONV_TILE_COUNTERS = 8192           # csrc/sr3_internal.h
SHAPE_COLUMNS = ["B", "H", "W", "Cin", "Cout", "ks", "stride", "up2", "stats", "precision"]
PLAN_COLUMNS = ["kernel", "tile_m", "tile_n", "split", "splits", "phases", "part_floats", "needs_counters", "stats_slices",
                "wino_ws_floats", "needs_wino_frag", "f8"]


def unet_convs(cfg, B, h, w):
    """(B, H, W, Cin, Cout, ks, stride, up2) of every conv launch of one UNet forward at h x w input pixels (unet.py:161-265;
    H, W = the conv's input size, Cin padded to 32 channels; a res_conv runs inside block2's launch and is not listed)."""
    pad32 = lambda c: (c + 31) // 32 * 32
    inner, n = cfg.inner_channel, len(cfg.channel_mults)
    out = [(B, h, w, pad32(cfg.in_channel), inner, 3, 1, 0)]

    def res(cin, cout, attn):
        out.append((B, h, w, pad32(cin), cout, 3, 1, 0))
        out.append((B, h, w, cout, cout, 3, 1, 0))
        if attn:
            out.append((B, h, w, cout, 3 * cout, 1, 1, 0))
            out.append((B, h, w, cout, cout, 1, 1, 0))

    pre, now_res = inner, cfg.image_size
    feat = [pre]
    for ind, mult in enumerate(cfg.channel_mults):
        attn = now_res in cfg.attn_res
        for _ in range(cfg.res_blocks):
            res(pre, inner * mult, attn)
            pre = inner * mult
            feat.append(pre)
        if ind != n - 1:
            out.append((B, h, w, pre, pre, 3, 2, 0))
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            feat.append(pre)
            now_res //= 2
    res(pre, pre, True)
    res(pre, pre, False)
    for ind in reversed(range(n)):
        attn = now_res in cfg.attn_res
        for _ in range(cfg.res_blocks + 1):
            res(pre + feat.pop(), inner * cfg.channel_mults[ind], attn)
            pre = inner * cfg.channel_mults[ind]
        if ind >= 1:
            out.append((B, h, w, pre, pre, 3, 1, 1))
            h, w = 2 * h, 2 * w
            now_res *= 2
    out.append((B, h, w, pre, cfg.out_channel, 3, 1, 0))
    return out


def shape_list():
    """[(B, H, W, Cin, Cout, ks, stride, up2, stats)], duplicates dropped, in a fixed order."""
    rows = []
    for size in (224, 128):                                   # the benchmark's UNets, 16 -> 128 pixels
        for B in (1, 4, 32, 64):
            rows += [s + (1,) for s in unet_convs(synth.yml_unet_config(size), B, 128, 128)]
    for B in (1, 2):                                          # smoke() and the tiny fixtures
        rows += [s + (1,) for s in unet_convs(synth.tiny_unet_config(), B, 16, 16)]
    for name, (B, H, W), _, _ in sweep.ROWS:
        rows += [s + (1,) for s in unet_convs(sweep._cfg(name), B, H, W)]
    for (B, H, W, Cin, Cout), *_ in gates.F32_CASES + gates.F16_CASES:
        rows.append((B, H, W, Cin, Cout, 3, 1, 0, 0))
    for B, H, W, C0, C1, Cout, ks, stride, up2 in ops.CONV_CASES:
        rows.append((B, H, W, C0 + C1, Cout, ks, stride, int(up2), 0))
    return list(dict.fromkeys(rows))


def plan_row(shape, prec):
    *conv, stats = shape
    d = engine.conv_plan(*conv, precision=prec, stats=bool(stats))
    return [d["kernel"], d["tile"][0], d["tile"][1], d["split"], d["splits"], d["phases"], d["part_floats"],
            int(d["needs_counters"]), d["stats_slices"], d["wino_ws_floats"], int(d["needs_wino_frag"]), int(d["f8"])]


def table_text():
    set_ = [s for s in SWITCHES if s in os.environ]
    assert not set_, f"the table is recorded with every conv switch unset; set: {set_}"
    lines = [json.dumps(list(shape) + [prec] + plan_row(shape, prec), separators=(",", ":"))
             for shape in shape_list() for prec in PRECISIONS]
    head = json.dumps({"columns": SHAPE_COLUMNS + PLAN_COLUMNS}, separators=(",", ":"))[1:-1]
    return "{" + head + ',\n"rows":[\n' + ",\n".join(lines) + "\n]}\n"


@pytest.fixture(scope="module")
def text():
    return table_text()


def test_library_reproduces_the_recorded_plans(text):
    with open(TABLE) as f:
        want = f.read()
    if text != want:
        got_rows, want_rows = json.loads(text)["rows"], json.loads(want)["rows"]
        diff = [(g, w) for g, w in zip(got_rows, want_rows) if g != w]
        assert len(got_rows) == len(want_rows), (len(got_rows), len(want_rows))
        assert not diff, f"{len(diff)} plans differ from tests/conv_plans.json; first (got, recorded): {diff[0]}"
    assert text == want


def test_plan_sizes_keep_their_promises(text):
    table = json.loads(text)
    assert table["columns"] == SHAPE_COLUMNS + PLAN_COLUMNS
    assert len(table["rows"]) > 1000
    seen = {"reduce": 0, "inplace": 0, "inplace_halo": 0, "up2": 0, "f8": 0}
    for row in table["rows"]:
        r = dict(zip(table["columns"], row))
        up = r["up2"]
        pad = r["ks"] // 2
        Ho = ((r["H"] << up) + 2 * pad - r["ks"]) // r["stride"] + 1
        Wo = ((r["W"] << up) + 2 * pad - r["ks"]) // r["stride"] + 1
        hw_phase = Ho * Wo // (4 if up else 1)                   # pixels of one image and phase
        M_phase = r["B"] * hw_phase
        assert r["phases"] == (4 if up and not r["kernel"].startswith("wino") else 1), row
        assert (r["splits"] > 1) == (r["split"] != "none"), row
        if r["splits"] > 1:
            assert r["part_floats"] == r["phases"] * r["splits"] * M_phase * r["Cout"], row
            seen[r["split"]] += 1
        else:
            assert r["part_floats"] == 0, row
        assert r["needs_counters"] == (r["split"] in ("inplace", "inplace_halo")), row
        if r["needs_counters"]:
            tiles = -(-M_phase // r["tile_m"]) * -(-r["Cout"] // r["tile_n"])
            assert tiles * r["phases"] <= CONV_TILE_COUNTERS, row
        if r["split"] == "inplace":
            assert r["kernel"] == "generic_64x64", row
        if r["split"] == "inplace_halo":
            assert r["kernel"] in ("halo_128x128_seg32", "halo_128x128_seg8") and r["precision"] != "f32", row
        if up:
            seen["up2"] += 1
            if r["split"] != "reduce":       # (a two-kernel split leaves the slices of its reduce pass)
                assert r["stats_slices"] == (4 * (r["H"] * r["W"] // r["tile_m"]) if r["H"] * r["W"] % r["tile_m"] == 0 else 0), row
        if r["f8"]:
            seen["f8"] += 1
            assert r["kernel"] == "halo_f8c" and r["splits"] == 1 and r["precision"] == "f16f8", row
        assert (r["kernel"] == "halo_f8c") == bool(r["f8"]), row
        assert (r["wino_ws_floats"] > 0) == (r["kernel"] == "wino_three_pass"), row
        assert bool(r["needs_wino_frag"]) == (r["kernel"] == "wino_one_pass"), row
        if r["kernel"].startswith(("wino", "halo")):
            assert r["kernel"].startswith("wino") == (r["precision"] == "f32"), row
    assert all(seen.values()), seen        # the list reaches every split kind, the upsample convs and the F8C path


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else TABLE
    with open(path, "w") as f:
        f.write(table_text())
    print(f"wrote {path}")
