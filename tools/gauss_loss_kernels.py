#!/usr/bin/env python3
"""The workload behind the kernel durations of DESIGN.md section 6n: update_model of a Gaussian FCModel at 256 envs x 128
steps (the size of section 6a's figures) under hyps["gauss_loss"] = "reference" and "exact", the two alternating in ONE
process on the same seeded data, so that one kernel trace holds a2c_gauss_loss_sums + a2c_gauss_loss_fwd_bwd
(gauss_sums_kernel, gauss_fwd_bwd_kernel) beside the a2c_gauss_nll_fwd_bwd (gauss_nll_kernel) that replaces them:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/gauss_loss_kernels.py --n 6
    python tools/kstats.py OUT 40

It times nothing itself; the rows of the three kernels in the profiler's statistics are the measurement.  --bandit instead
plays the one-state bandit of tests/test_gpu_gauss_exact.py under both losses and prints |mu - 1.5| before and after."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-a2c_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def hyps_for(mode, R, T, **kw):
    return dict(dict(gamma=.99, lambda_=.98, n_tsteps=T, n_rollouts=R, use_bptt=False, use_nstep_rets=False, norm_advs=True,
                     entr_coef=.005, pi_coef=1.0, val_coef=.5, max_norm=.5, lr=1e-4, optim_type="RMSprop", is_discrete=False,
                     gauss_loss=mode), **kw)


def updates(n, R, T, h, rounds):
    import torch
    import a2c_amd
    from a2c_amd.updater import Updater
    N = R * T
    g = torch.Generator().manual_seed(1)
    dones = (torch.rand(N, generator=g) < 0.02).float()
    dones[T - 1::T] = 1.0
    D = {k: v.cuda() for k, v in dict(states=torch.randn(N, 4, 1, 4, generator=g), actions=torch.randn(N, n, generator=g),
                                      rewards=torch.randn(N, generator=g), deltas=torch.randn(N, generator=g), dones=dones).items()}
    upds = {}
    for mode in ("reference", "exact"):
        torch.manual_seed(0)
        net = a2c_amd.FCModel([4, 1, 4], n, h_size=h, is_discrete=False).cuda()
        upds[mode] = Updater(net, hyps_for(mode, R, T))
    infos = {}
    for _ in range(rounds):
        for mode, upd in upds.items():
            infos[mode] = upd.update_model(D)
    torch.cuda.synchronize()
    return dict(n=n, rows=N, h=h, updates_per_mode=rounds, last_info=infos)


def bandit(n, seed, mode, rows=256, n_updates=60, target=1.5):
    import torch
    import a2c_amd
    from a2c_amd import ops
    from a2c_amd.updater import Updater
    torch.manual_seed(seed)
    net = a2c_amd.FCModel([1, 1, 8], n, h_size=32, is_discrete=False).cuda()
    upd = Updater(net, hyps_for(mode, 1, rows, gamma=0.0, lambda_=0.0, lr=1e-3, entr_coef=.001))
    states = torch.full((rows, 1, 1, 8), 0.25, device="cuda")
    dones = torch.zeros(rows, device="cuda")
    dones[-1] = 1.0
    eps = torch.randn(n_updates, rows, n, generator=torch.Generator().manual_seed(100 + seed)).cuda()
    acts = torch.zeros(rows, n, device="cuda")

    def miss():
        with torch.no_grad():
            return float((net(states)[1][0] - target).abs().max())
    start = miss()
    for k in range(n_updates):
        with torch.no_grad():
            v = net(states)[0].view(-1).clone()
        ops.gauss_head(net._heads("pub", rows)[1], n, rows, eps=eps[k], actions_ptr=acts.data_ptr(), act_ld=n)
        r = -((acts - target) ** 2).sum(dim=1)
        upd.update_model(dict(states=states, actions=acts, rewards=r, dones=dones, deltas=r - v))
    return dict(n=n, seed=seed, gauss_loss=mode, start=round(start, 4), end=round(miss(), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=6, help="action dimension")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--tsteps", type=int, default=128)
    ap.add_argument("--h", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=50, help="updates per mode (the first ones warm up; the trace's mean is over all)")
    ap.add_argument("--bandit", action="store_true")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "gauss_loss_kernels needs the MI355X"
    if args.bandit:
        for n in (1, 2):
            for seed in (0, 1, 2):
                for mode in ("reference", "exact"):
                    print(json.dumps(bandit(n, seed, mode)), flush=True)
        return
    print(json.dumps(updates(args.n, args.envs, args.tsteps, args.h, args.rounds)))


if __name__ == "__main__":
    main()
