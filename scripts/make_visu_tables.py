#!/usr/bin/env python3
"""Write the colour tables that ship inside wild_visual_navigation_amd/visu/ (needs matplotlib; run once, commit the output):

    python scripts/make_visu_tables.py [--check]

  rdylbu_stretched_256.txt  visualizer.py:379-384 of the reference (plot_detectron_classification's default), then the
                            conversion of plot_segmentation (:505): fp32 table, (c * 255) truncated to uint8
  rdylbu_256.txt            sns.color_palette("RdYlBu", 256) by seaborn's sampling rule on matplotlib (visu/colormaps.py), converted alike
  rdylbu_graph_256.txt      visualizer.py:458-459 of the reference (plot_graph_result): the map resampled to 255 entries, sampled at
                            linspace(0, 1, 256), np.uint8(c * 255) in float64

--check compares the files with what matplotlib gives now and exits 1 on a difference."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "wild_visual_navigation_amd", "visu")


def to_u8(c):
    return (np.asarray(c, dtype=np.float32)[:, :3] * np.float32(255)).astype(np.uint8)


def stretched_rdylbu():
    import matplotlib

    s = 0.3
    cmap = matplotlib.colormaps["RdYlBu"].resampled(256)   # cm.get_cmap("RdYlBu", 256)
    return to_u8(np.concatenate([cmap(np.linspace(0, s, 128)), cmap(np.linspace(1 - s, 1.0, 128))]))


def graph_result_rdylbu():
    import matplotlib

    cmap = matplotlib.colormaps["RdYlBu"].resampled(255)   # cm.get_cmap("RdYlBu", 255)
    return np.uint8(cmap(np.linspace(0, 1, 256))[:, :3] * 255)


def tables():
    from wild_visual_navigation_amd.visu.colormaps import sample_matplotlib

    return {"rdylbu_stretched_256.txt": stretched_rdylbu(), "rdylbu_256.txt": to_u8(sample_matplotlib("RdYlBu", 256)),
            "rdylbu_graph_256.txt": graph_result_rdylbu()}


def main():
    check = "--check" in sys.argv
    bad = 0
    for name, t in tables().items():
        text = "".join(f"{r} {g} {b}\n" for r, g, b in t.tolist())
        path = os.path.join(OUT, name)
        if check:
            same = os.path.exists(path) and open(path).read() == text
            print(f"{name}: {'ok' if same else 'DIFFERS'}")
            bad += not same
        else:
            with open(path, "w") as f:
                f.write(text)
            print(f"wrote {path} ({len(t)} entries)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
