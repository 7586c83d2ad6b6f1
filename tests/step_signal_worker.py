"""Plan-step runs for tests/test_gpu_step_signals.py: race_worker's shapes and seeds (H = d = 64,
E = 48, 40 users, 60 tracks, 5 steps, flush_every 3), with the options that test needs on top --
steps without an announced next batch, and batches staged into reused device buffers behind a sleep
on the caller's stream.

Run as a script it makes the runs named on the command line in this process -- the parent sets
DCUE_XQ_WAIT=event, or one of the group switches DCUE_XQ_START / DCUE_XQ_FORK / DCUE_XQ_LATE to 0,
which the library reads once at load -- and saves them to a file:

  python step_signal_worker.py OUT.pt bn,cat,text,small,nonext
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "amplifai-deepcontentrecommenders_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from race_worker import DEV, TOWERS, finite, same  # noqa: E402,F401

SLEEP_CYCLES = 12_000_000  # about 5 ms of torch.cuda._sleep at 2.4 GHz

# the runs of the mode comparison: name -> run() arguments
CASES = {
    "bn": dict(tower="bn"),
    "cat": dict(tower="bn", inbatch=False),  # M = B (1 + N) = 96
    "text": dict(tower="text"),
    "small": dict(tower="bn", B=4, N=2),  # dgrad 4 and dgrad 3 are one workgroup each
    "nonext": dict(tower="bn", set_next=False),  # no lookahead: k_input_stats starts the step
}


def run(tower="bn", delays=None, steps=5, inbatch=True, B=16, N=5, set_next=True, staged=False):
    """Steps of one fresh model. delays: {site: microseconds}. staged: before each step the caller's
    stream sleeps ~5 ms, then that step's users (and items) are copied into reused device buffers
    and the step runs from those. Returns loss / P / emb (CPU) and the library's launch count."""
    from dcrecommend import _native as nat
    from dcrecommend.dcue.dcue import DCUENet
    from dcrecommend.dcue.plan import TrainPlan
    from dcrecommend.optim import NativeAdam
    n_users, n_tracks = 40, 60
    args = dict(TOWERS[tower], user_embdim=48, user_count=n_users)
    torch.manual_seed(0)
    net = DCUENet(args).to(DEV).train()
    opt = NativeAdam(net.parameters(), 1e-3, (0.9, 0.99), 1e-8, 0, defer_embedding=True, flush_every=3)
    gen = torch.Generator().manual_seed(1)
    X = torch.randn(n_tracks, 128, 131, generator=gen).half()
    table = X.transpose(1, 2).contiguous().to(DEV)
    tokens = None
    if tower.startswith("text"):
        from oracle import text_oracle as TO
        tokens = TO.sentences(gen, n_tracks, args["text_len"], args["n_words"], args["pad_idx"]).to(DEV)
    M = B if inbatch else B * (1 + N)
    users = [torch.randint(0, n_users, (B,), generator=gen).to(DEV) for _ in range(steps + 1)]
    items = [torch.randint(0, n_tracks, (M,), generator=gen).to(torch.int32).to(DEV) for _ in range(steps + 1)]
    if inbatch:
        mt = torch.empty(nat.MT_STATE_BYTES, dtype=torch.uint8, device=DEV)
        nat.check(nat.lib().dcue_mt_seed(nat.ptr(mt), 7, nat.stream_handle()), "mt_seed")
        plan = TrainPlan(net, table, B, N, mt_state=mt, optimizer=opt, tokens=tokens)
    else:
        plan = TrainPlan(net, table, B, N, item_track=items[0], optimizer=opt, tokens=tokens)
    look = inbatch and set_next
    # staged: one users buffer, rewritten behind the sleep right before its step. Items: an announced
    # batch must keep its contents until its step has run, so with the lookahead they go through a
    # ring of three buffers (written one step ahead, behind the sleep, before they are announced);
    # without it, through one buffer rewritten right before its step, as the users
    ubuf = torch.zeros_like(users[0])
    ibuf = [torch.zeros_like(items[0]) for _ in range(3 if look else 1)]
    if staged and look:
        ibuf[0].copy_(items[0])
    torch.cuda.synchronize()
    for site, us in (delays or {}).items():
        nat.debug_delay(site, us)
    l0 = nat.lib().dcue_launch_count()
    losses = []
    try:
        for s in range(steps):
            if staged:
                torch.cuda._sleep(SLEEP_CYCLES)
                ubuf.copy_(users[s])
                if look:
                    ibuf[(s + 1) % 3].copy_(items[s + 1])
                    plan.set_next(ibuf[(s + 1) % 3])
                    plan.step(ubuf, ibuf[s % 3])
                else:
                    ibuf[0].copy_(items[s])
                    plan.step(ubuf, ibuf[0])
            else:
                if look:
                    plan.set_next(items[s + 1])
                plan.step(users[s], items[s])
            losses.append(plan.loss.detach().clone())
        torch.cuda.synchronize()
    finally:
        nat.debug_clear_delays()
    launches = nat.lib().dcue_launch_count() - l0
    opt.flush()
    sd = net.state_dict()
    out = {"loss": torch.stack(losses).cpu(), "P": net._flat["P"].detach().cpu(),
           "emb": sd["user_embd.embeddings.weight"].cpu(), "launches": int(launches)}
    plan.close()
    torch.cuda.synchronize()
    return out


def main():
    from dcrecommend import _native as nat
    out_path, names = sys.argv[1], sys.argv[2].split(",")
    res = {n: run(**CASES[n]) for n in names}
    torch.save(res, out_path)
    print(json.dumps({"xq_wait": os.environ.get("DCUE_XQ_WAIT", ""),
                      "xq_groups": {g: os.environ.get("DCUE_XQ_" + g, "") for g in ("START", "FORK", "LATE")},
                      "fail_flags": int(nat.debug_fail_flags()),
                      "finite": {n: finite(r) for n, r in res.items()}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
