#!/usr/bin/env python3
"""One data-parallel rank of ONE accumulated window of the product step (MAEPretrainModule.fused_training_step with
``accumulate=(index, count)``), started as a fresh child process by tests/test_gpu_accumulate_dp.py.  Every rank uses cuda:0 and the
gloo backend, as tests/dp_worker.py.  The window's global micro-batches hold ``--rows`` rows (default 4,3,1); rank r takes rows
[ceil(n r / W), ceil(n (r + 1) / W)) of each, so the last rank's share of a one-row micro-batch is empty.  The noise is drawn once
for the window's rows.  With --world 1 it is the single-process window.

    python tests/accum_dp_worker.py --rank 0 --world 2 --port 29511 --out /tmp/x
"""
import argparse
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--port", type=int, default=29511)
    ap.add_argument("--out", required=True)
    ap.add_argument("--rows", default="4,3,1")
    a = ap.parse_args()

    import torch
    import torch.distributed as dist
    from ssrl_vit_mae_jepa_amd import MAEPretrainModule
    from ssrl_vit_mae_jepa_amd import dist as mdist

    if a.world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port), RANK=str(a.rank), WORLD_SIZE=str(a.world), LOCAL_RANK="0")
        dist.init_process_group("gloo")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    general = dict(image_size=32, patch_size=8, in_chans=3, mask_ratio=0.75, engine_precision="fp32")
    encoder, decoder = dict(embed_dim=48, depth=3, num_heads=2), dict(decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2)
    tcfg = dict(mask_ratio_start=0.75, mask_ratio_end=0.75, mask_ramp_epochs=5, total_epochs=800, warmup_epochs=20,
                batch_size=2000, base_learning_rate=1.5e-4, weight_decay=0.05)
    module = MAEPretrainModule(dict(general=general, encoder=encoder, decoder=decoder), tcfg)
    net = module.model
    net._init_weights(seed=73)  # identical parameters on every rank
    with torch.no_grad():
        g = torch.Generator().manual_seed(7)
        for n, p in net.named_parameters():
            if p.requires_grad and p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    module = module.to(dev)
    module.on_train_epoch_start()
    split = [int(v) for v in a.rows.split(",")]
    total = sum(split)
    images = (torch.rand(total, 3, 32, 32, generator=torch.Generator().manual_seed(100)) * 2 - 1).to(dev)
    noise = mdist.global_noise(total, net.sequence_length, 73, module.global_step, dev)   # once per window
    full_loss = net.loss_and_grads(images, noise).clone() if a.world == 1 else torch.zeros(1)   # the whole window as one batch: what its mean loss must be
    losses, my_rows, before = [], [], 0
    for i, n in enumerate(split):
        lo, hi = before + -(-n * a.rank // a.world), before + -(-n * (a.rank + 1) // a.world)
        my_rows.append(hi - lo)
        losses.append(module.fused_training_step(images[lo:hi].contiguous(), noise[lo:hi].contiguous(), global_rows=total,
                                                 accumulate=(i, len(split))).clone())
        before += n
    torch.cuda.synchronize()
    if a.world > 1:
        module.gather_optimizer_state()
    out = {"params": net.flat_params.detach().cpu(), "losses": torch.cat(losses).cpu(), "rows": torch.tensor(my_rows), "full_loss": full_loss.cpu(),
           "exp_avg": module._exp_avg.detach().cpu(), "stats": module._stats.cpu(), "steps": torch.tensor([module.global_step, module._opt_steps]),
           "buckets": module.gradient_buckets() if a.world > 1 else [], "overlap": module.overlap_exchange}
    torch.save(out, f"{a.out}/w{a.world}_r{a.rank}.pt")
    if a.world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
