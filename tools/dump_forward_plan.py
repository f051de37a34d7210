#!/usr/bin/env python3
"""What the forward's kernel chooser answers, as JSON lines: for a chooser refactor, run it on the build before and on the build
after and compare the two outputs byte for byte (host-only entry points of the library: no GPU needed).

    python tools/dump_forward_plan.py > plan.jsonl

One line per configuration of the full product of: model variant, precision (f32, f32_split, f16), activations kept or not,
up-sampling on read, the wide 3x3 form, each stem fusion, latency mode (off / more cells than the batch has) and the shapes the
tests assert kernel names on.  A line holds, per layer, (name, bm, bn, algo) of om_layer_tile (om_layer_tile_f16 for f16), the
workspace sizes, the status word's offset and, with activations kept, every layer's om_layer_output_view tuple.
"""
import ctypes
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orienmask_amd import lib, pack  # noqa: E402

# tests/test_host_cpu.py::test_layer_audit_covers_every_chooser_kernel's shapes, then the other shapes of the GPU tests' kernel names
SHAPES = [(32, 544, 544), (64, 544, 544), (1, 544, 544), (6, 544, 544), (1, 160, 128), (2, 320, 416),
          (140, 32, 544), (3, 32, 544), (2, 160, 224), (7, 544, 544), (2, 544, 544), (8, 544, 544)]


def main():
    L = lib.load()
    chk = lib.check
    old = (L.om_get_wino14_wide(), L.om_get_stem_fusion(0), L.om_get_stem_fusion(1))
    for variant in (0, 1):
        h = ctypes.c_void_p()
        chk(L.om_model_create_variant(ctypes.byref(h), variant, 3, 80), "om_model_create_variant")
        n = L.om_model_num_layers(h)
        names = [l["name"] for l in pack.graph_layers(h)]
        for precision, keep, uor, wide, stem3, stem2h, latency, (B, H, W) in itertools.product(
                ("f32", "f32_split", "f16"), (0, 1), (1, 0), (1, 0), (1, 0), (1, 0), (0, 1), SHAPES):
            chk(L.om_model_set_precision(h, 1 if precision == "f32_split" else 0), "om_model_set_precision")
            chk(L.om_model_keep_activations(h, keep), "om_model_keep_activations")
            chk(L.om_model_set_upsample_on_read(h, uor), "om_model_set_upsample_on_read")
            chk(L.om_set_wino14_wide(wide), "om_set_wino14_wide")
            chk(L.om_set_stem_fusion(0, stem3), "om_set_stem_fusion")
            chk(L.om_set_stem_fusion(1, stem2h), "om_set_stem_fusion")
            cells = B * (H // 32) * (W // 32) + 1 if latency else 0
            chk(L.om_model_set_latency_cells(h, cells), "om_model_set_latency_cells")
            f16 = precision == "f16"
            tile = L.om_layer_tile_f16 if f16 else L.om_layer_tile
            layers = []
            for i in range(n):
                bm, bn, algo = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
                chk(tile(h, i, B, H, W, ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(algo)), "om_layer_tile")
                layers.append((names[i], bm.value, bn.value, algo.value))
            views = None
            if keep:
                views = []
                for i in range(n):
                    off, ch, ps, div = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
                    rc = L.om_layer_output_view(h, i, B, H, W, 1 if f16 else 0, ctypes.byref(off), ctypes.byref(ch),
                                                ctypes.byref(ps), ctypes.byref(div))
                    views.append((off.value, ch.value, ps.value, div.value) if rc == 0 else None)      # None: a caller-owned head tensor
            print(json.dumps({
                "variant": variant, "precision": precision, "keep_activations": keep, "upsample_on_read": uor, "wino14_wide": wide,
                "stem3": stem3, "stem2_f16": stem2h, "latency_cells": cells, "shape": (B, H, W), "layers": layers,
                "workspace_bytes": L.om_forward_workspace_bytes(h, B, H, W),
                "f16_workspace_bytes": L.om_forward_f16_workspace_bytes(h, B, H, W),
                "status_offset": L.om_forward_status_offset(h, B, H, W), "views": views}, separators=(",", ":")))
        L.om_model_destroy(h)
    L.om_set_wino14_wide(old[0])
    L.om_set_stem_fusion(0, old[1])
    L.om_set_stem_fusion(1, old[2])


if __name__ == "__main__":
    main()
