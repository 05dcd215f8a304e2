"""Per-segment traversability inference (prediction_per_pixel = False): FeatureExtractor.predict_per_segment (extract_batch ->
csrc/segment_predict.hip) beside the caller-side sequence of quick_start.py:184-210 / wvn_feature_extractor_node.py:320-366 on the
same library (extract_batch -> per frame feat[seg] gather -> SimpleMLP.forward -> column 0 / confidence).  Synthetic ViT-S/8
weights.  One JSON line per case, times in ms per frame: whole call ("*_ms_per_frame") and the part after extract_batch
("*_tail_ms_per_frame").

    python scripts/bench_segment_predict.py [--cases 224x1:grid,448x64:grid,448x64:stego] [--iters N]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wild_visual_navigation_amd.backbone import synthetic_vit_state_dict  # noqa: E402
from wild_visual_navigation_amd.cfg import ExperimentParams  # noqa: E402
from wild_visual_navigation_amd.feature_extractor import FeatureExtractor  # noqa: E402
from wild_visual_navigation_amd.model import get_model  # noqa: E402
from wild_visual_navigation_amd.utils import ConfidenceGenerator, Data  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def run_case(dev, size, B, seg_type, iters):
    ftype = "stego" if seg_type == "stego" else "dino"
    fe = FeatureExtractor(device=dev, segmentation_type=seg_type, feature_type=ftype, patch_size=8, backbone_type="vit_small",
                          input_size=size, pretrained_weights=synthetic_vit_state_dict(depth=12, pretrain_grid=28),
                          n_image_clusters=20, run_clustering=True)
    params = ExperimentParams()
    params.model.simple_mlp_cfg.input_size = fe.feature_dim
    model = get_model(params.model).to(dev)
    model.eval()
    cg = ConfidenceGenerator(method="latest_measurement", std_factor=0.5).to(dev)
    cg.mean[0], cg.std[0] = 0.9, 0.25
    frames = torch.randint(0, 256, (B, 3, size, size), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)

    def sequence_tail(feat, seg, nseg):
        out = []
        for b in range(B):   # the callers run one frame at a time; a batched gather would need B x 308 MB at 448^2
            x = feat[b][seg[b].reshape(-1).long()]
            pred = model.forward(Data(x=x))
            mse = ((pred[:, 1:] - x) ** 2).mean(1)
            out.append((pred[:, 0].reshape(size, size), cg.inference_without_update(mse).reshape(size, size)))
        return out

    def sequence():
        return sequence_tail(*fe.extract_batch(frames))

    extracted = fe.extract_batch(frames)
    feat, seg, _ = extracted
    conf_state = torch.tensor([0.9, 0.25, 0.5], dtype=torch.float32, device=dev)
    fused_ms = timed(lambda: fe.predict_per_segment(frames, model, cg), iters) / B
    seq_ms = timed(sequence, iters) / B
    extract_ms = timed(lambda: fe.extract_batch(frames), iters) / B
    fused_tail_ms = timed(lambda: model.forward_per_segment(feat, seg, conf_state=conf_state), iters) / B
    seq_tail_ms = timed(lambda: sequence_tail(*extracted), iters) / B
    # the two paths on the same extract_batch output
    trav, conf, _ = model.forward_per_segment(feat, seg, conf_state=conf_state)
    ref = sequence_tail(*extracted)
    err_t = max(float((trav[b] - ref[b][0]).abs().max()) for b in range(B))
    err_c = max(float((conf[b] - ref[b][1]).abs().max()) for b in range(B))
    return {"frame": f"{size}x{size}", "batch": B, "segmentation": seg_type, "feature_type": ftype, "segments": int(feat.shape[1]),
            "fused_ms_per_frame": round(fused_ms, 4), "sequence_ms_per_frame": round(seq_ms, 4),
            "extract_batch_ms_per_frame": round(extract_ms, 4),
            "fused_tail_ms_per_frame": round(fused_tail_ms, 5), "sequence_tail_ms_per_frame": round(seq_tail_ms, 4),
            "speedup": round(seq_ms / fused_ms, 2), "tail_speedup": round(seq_tail_ms / fused_tail_ms, 1),
            "max_abs_diff_trav": err_t, "max_abs_diff_conf": err_c}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="224x1:grid,448x64:grid,448x64:stego", help="SIZExBATCH:SEGMENTATION, comma-separated")
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for case in args.cases.split(","):
        shape, seg_type = case.split(":")
        size, B = (int(v) for v in shape.split("x"))
        print(json.dumps(run_case(dev, size, B, seg_type, args.iters)), flush=True)


if __name__ == "__main__":
    main()
