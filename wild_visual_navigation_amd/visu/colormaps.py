"""Colour tables of the overlays.

Two tables ship as data files (256 lines "r g b", uint8; scripts/make_visu_tables.py writes them from matplotlib), so that the
default pictures need no plotting package at run time:

  rdylbu_stretched_256.txt   the default of plot_detectron_classification (visualizer.py:379-384 of the reference): matplotlib's
                             "RdYlBu" resampled to 256 entries, [cmap(linspace(0, s, 128)) | cmap(linspace(1 - s, 1, 128))],
                             s = 0.3, as fp32, (c * 255) truncated to uint8
  rdylbu_256.txt             sns.color_palette("RdYlBu", 256): the default ``colormap`` of plot_traversability_graph_on_seg,
                             plot_mission_node_prediction / _training -- by seaborn's sampling rule, see below

  rdylbu_graph_256.txt       the table of plot_graph_result (visualizer.py:458-459 of the reference): matplotlib's "RdYlBu"
                             resampled to 255 entries, sampled at linspace(0, 1, 256), (c * 255) truncated to uint8

Any other name resolves through seaborn when it is importable, otherwise through matplotlib with seaborn's sampling rule
(seaborn.palettes.mpl_palette): a qualitative map's colours cycled to n entries, any other map sampled at the interior points
of linspace(0, 1, n + 2).  UNPINNED: seaborn is not installed where this was written, so that rule is taken from seaborn's
published source and not compared against it."""
import os

import torch

from .._lib import WvnError

_HERE = os.path.dirname(os.path.abspath(__file__))
_PACKAGED = {("RdYlBu", 256): "rdylbu_256.txt"}
_DEFAULT = "rdylbu_stretched_256.txt"
_GRAPH_RESULT = {"RdYlBu": "rdylbu_graph_256.txt"}
# matplotlib's qualitative maps and the number of colours seaborn takes from each (seaborn.palettes.MPL_QUAL_PALS)
QUALITATIVE = {"tab10": 10, "tab20": 20, "tab20b": 20, "tab20c": 20, "Set1": 9, "Set2": 8, "Set3": 12, "Accent": 8, "Paired": 12,
               "Pastel1": 9, "Pastel2": 8, "Dark2": 8}
_cache = {}


def _read(name: str) -> torch.Tensor:
    if name not in _cache:
        with open(os.path.join(_HERE, name)) as f:
            rows = [[int(v) for v in ln.split()] for ln in f if ln.strip() and not ln.startswith("#")]
        t = torch.tensor(rows, dtype=torch.uint8)
        if t.dim() != 2 or t.shape[1] != 3:
            raise WvnError(f"{name}: not an [N,3] colour table")
        _cache[name] = t
    return _cache[name]


def default_classification_table() -> torch.Tensor:
    """uint8 [256,3] on the CPU: the stretched RdYlBu table of plot_detectron_classification."""
    return _read(_DEFAULT)


def sample_matplotlib(name: str, n: int):
    """seaborn's mpl_palette on matplotlib alone -> float64 numpy [n,3]."""
    try:
        import matplotlib
        import numpy as np
    except ImportError as e:
        raise WvnError(f"colour map {name!r} ({n} entries) is not packaged: it needs seaborn or matplotlib, neither is installed") from e
    try:
        cmap = matplotlib.colormaps[name]
    except KeyError as e:
        raise WvnError(f"colour map {name!r} is not packaged, seaborn is not installed, and matplotlib does not know the name") from e
    if name in QUALITATIVE:
        base = cmap(np.linspace(0, 1, QUALITATIVE[name]))[:, :3]
        return np.stack([base[i % len(base)] for i in range(n)])
    return cmap(np.linspace(0, 1, int(n) + 2)[1:-1])[:, :3]


def colour_table(name: str, n: int) -> torch.Tensor:
    """``sns.color_palette(name, n)`` as a CPU tensor [n,3]: uint8 for a packaged table, else fp32 in [0,1] (what
    ``torch.tensor(sns.color_palette(...))`` gives; the kernel converts it with the reference's (c * 255) -> uint8)."""
    n = int(n)
    if (name, n) in _PACKAGED:
        return _read(_PACKAGED[(name, n)])
    key = ("named", name, n)
    if key not in _cache:
        try:
            import seaborn as sns
        except ImportError:
            pal = sample_matplotlib(name, n)
        else:
            pal = sns.color_palette(name, n)
        _cache[key] = torch.tensor([[float(v) for v in c[:3]] for c in pal], dtype=torch.float32)
    return _cache[key]


def graph_result_table(name: str = "RdYlBu") -> torch.Tensor:
    """uint8 [256,3] on the CPU: ``np.uint8(cm.get_cmap(name, 255)(np.linspace(0, 1, 256))[:, :3] * 255)`` of plot_graph_result.
    "RdYlBu" is packaged; any other name needs matplotlib (``matplotlib.colormaps[name].resampled(255)`` is the same construction)."""
    if name in _GRAPH_RESULT:
        return _read(_GRAPH_RESULT[name])
    key = ("graph_result", name)
    if key not in _cache:
        try:
            import matplotlib
            import numpy as np
        except ImportError as e:
            raise WvnError(f"colour map {name!r} of plot_graph_result is not packaged: it needs matplotlib, which is not installed") from e
        try:
            cmap = matplotlib.colormaps[name].resampled(255)
        except KeyError as e:
            raise WvnError(f"colour map {name!r} is not packaged and matplotlib does not know the name") from e
        _cache[key] = torch.from_numpy(np.uint8(cmap(np.linspace(0, 1, 256))[:, :3] * 255))
    return _cache[key]
