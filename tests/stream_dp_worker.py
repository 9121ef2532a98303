"""Worker of tests/test_hip_streams.py::test_two_ranks_one_gpu: ONE rank of a 2-rank data-parallel run of a stream
pre-training step (spatialstream / temporalstream ``VGG``: train-mode encoder without autograd, decoder forward / backward,
floss, FusedAdam over the decoder + dp.GradReducer).  Both ranks share GPU 0 and exchange gradients over gloo.
argv: out-prefix stream.  Launched by torch.distributed.run; writes its observations to argv[1].<rank>."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out_prefix, stream = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import egaze_amd  # noqa: F401
    import egaze_amd.hipops as H
    from egaze_amd import dp, streams, streamtrain, synthetic
    from egaze_amd.floss import floss
    from egaze_amd.optim import FusedAdam
    from egaze_amd.utils import cfg, make_layers

    torch.manual_seed(1234)                              # the same encoder on every rank (it is never broadcast: frozen)
    model = streamtrain.StreamVGG(make_layers(cfg['D'], 3 if stream == "spatial" else 20),
                                  freeze_features=stream == "spatial").to(dev)
    with torch.no_grad():                                # ... but the decoders start DIFFERENT: attach() must broadcast rank 0's
        for p in model.decoder.parameters():
            p.add_(1e-3 * rank)
    model.train()
    crit = floss().to(dev)
    opt = FusedAdam(model.decoder.parameters(), lr=1e-4)
    b = synthetic.sp_batch(2, 32, dev, seed=100 + rank)
    x = b["image"] if stream == "spatial" else b["flow"]
    enc0 = torch.cat([p.detach().reshape(-1) for p in model.features.parameters()]).cpu()

    def fwd_bwd():
        opt.zero_grad()
        out = streamtrain.step_forward(model, x)
        loss = crit(out, b["gt"].view(out.size()))
        loss.backward()
        return loss

    # (0) identical replicas first (what dp.attach does), then the LOCAL gradient without a reducer
    flat = opt.flat_p.detach().cpu()
    dist.broadcast(flat, src=0)
    opt.flat_p.copy_(flat)
    H.bump_weight_epoch()
    fwd_bwd()
    streams.join_all_into_current()
    torch.cuda.synchronize()
    g_local = opt.flat_g.detach().cpu().clone()
    gathered = [torch.empty_like(g_local) for _ in range(world)]
    dist.all_gather(gathered, g_local)

    # (1) the same backward with the reducer attached
    red = dp.attach(opt, bucket_bytes=8 * 1024 * 1024)
    fwd_bwd()
    red.wait()
    torch.cuda.synchronize()
    g_sum = opt.flat_g.detach().cpu().clone()

    # (2) two optimizer steps through the normal path
    losses = []
    for _ in range(2):
        loss = fwd_bwd()
        opt.step()
        losses.append(loss.item())
    torch.cuda.synchronize()
    enc = torch.cat([p.detach().reshape(-1) for p in model.features.parameters()]).cpu()
    torch.save({"rank": rank, "g_local": gathered, "g_sum": g_sum, "flat_p": opt.flat_p.detach().cpu().clone(),
                "losses": losses, "n_buckets": len(red.buckets), "grad_scale": opt.grad_scale, "enc": enc, "enc0": enc0,
                "enc_grads_none": all(p.grad is None for p in model.features.parameters())},
               f"{out_prefix}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
