"""SAM predictor timing on one MI355X (profiles/sam_predictor.md): the two prompt-encoder kernels and `predict_torch` at b = 1 and 64, with and without
`mask_input`, HIP events after warm-up.  Random weights (the time does not depend on the values), a 1024 x 1024 original image, the embedding set by hand:
the image encoder is not part of a prediction.
usage: python tools/sam_predictor_bench.py [out.md]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llmseg_amd import ops  # noqa: E402
from llmseg_amd.lisa import LISAForCausalLM  # noqa: E402
from llmseg_amd.params import LisaConfig, LlamaConfig, SamConfig, VitConfig  # noqa: E402

PE = "model.visual_model.prompt_encoder."
dev = torch.device("cuda:0")
cfg = LisaConfig(backbone="sam", build_unused_towers=False, sam_decoder=True, sam_prompts=True)
cfg.llama, cfg.clip, cfg.sam = LlamaConfig(layers=1), VitConfig(layers=1), SamConfig(dim=160, depth=2, heads=2, global_idx=(1,))
m = LISAForCausalLM(cfg, device=dev).init_random(seed=0)
p = m.predictor()
p.features = torch.randn(4096, 256, device=dev).to(torch.bfloat16)
p.input_size, p.original_size, p.is_image_set = (1024, 1024), (1024, 1024), True
P, S = m.params, m._samdec()


def timed(fn, warmup=5, iters=30):
    """median and minimum of `iters` event-timed calls, in microseconds"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


lines = ["| what | b | median us | min us | note |", "|---|---|---|---|---|"]
for b in (1, 64):
    coords = torch.rand(b, 2, 2, device=dev) * 1024
    labels = torch.ones(b, 2, device=dev, dtype=torch.int32)
    boxes = torch.rand(b, 4, device=dev) * 1024
    mask = (torch.rand(b, 65536, device=dev) * 40 - 20).contiguous()
    keys = torch.empty((b * 4096, 256), device=dev, dtype=torch.bfloat16)
    emb = [P[f"{PE}point_embeddings.{i}.weight"] for i in range(4)]
    W = m.mask_downscaling_weights()
    mb = b * 4096 * 256 * 2 / 1e6
    for nested in (True, False):
        med, mn = timed(lambda: ops.sam_dense_prompt(p.features, mask, weights=W, nested=nested, out=keys))
        lines.append(f"| llmseg_sam_dense_prompt, mask {'nested' if nested else 'raster'} | {b} | {med:.1f} | {mn:.1f} | {mb:.1f} MB stored, {mb * 1e6 / (med * 1e-6) / 1e12:.2f} TB/s at the median |")
    med, mn = timed(lambda: ops.sam_dense_prompt(p.features, None, no_mask=P[PE + "no_mask_embed.weight"], b=b, out=keys))
    lines.append(f"| llmseg_sam_dense_prompt, mask NULL | {b} | {med:.1f} | {mn:.1f} | {mb:.1f} MB stored, {mb * 1e6 / (med * 1e-6) / 1e12:.2f} TB/s at the median |")
    med, mn = timed(lambda: ops.add_rows(p.features.repeat(b, 1) if b > 1 else p.features, P[PE + "no_mask_embed.weight"], out=keys))
    lines.append(f"| add_rows(feats.repeat(b, 1), no_mask) (the route without the kernel) | {b} | {med:.1f} | {mn:.1f} | |")
    med, mn = timed(lambda: ops.sam_prompt_tokens(coords, labels, boxes, S["G"], emb, P[PE + "not_a_point_embed.weight"]))
    lines.append(f"| llmseg_sam_prompt_tokens, 2 points + box | {b} | {med:.1f} | {mn:.1f} | includes the output allocation |")
    for tag, kw in (("points + box", {}), ("points + box + mask_input (nested)", dict(mask_input=mask))):
        for mm in (True, False):
            med, mn = timed(lambda: p.predict_torch(coords, labels, boxes, multimask_output=mm, low_res_nested=True, **kw), warmup=3, iters=10)
            lines.append(f"| predict_torch, {tag}, multimask_output={mm} | {b} | {med:.0f} | {mn:.0f} | decoder + post-processing to 1024 x 1024 |")
text = "\n".join(lines)
print(text)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write(text + "\n")
