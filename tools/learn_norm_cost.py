"""Cost of the learner's two actor-critic options at the headline shape:

    python tools/learn_norm_cost.py [--out profiles/learn_norm_cost.txt] [--rounds 10] [--inner 20]

One process on one MI355X, the bench's cfg 2 model and B = 256 trajectories of 16 frames: one rollout, then the learner step alone (d4_learn through
run_learner: losses and the gradients of both heads, no optimiser) with the options off, each on, and both on.  The four variants alternate within
every round (A/B in one process, so that drift and other tenants hit all alike); a round times `inner` steps of each between device events after a
warm-up of every variant; the table gives the median, the minimum and the spread over the rounds.  The return statistics kernel runs on all
4096 rows (one workgroup); the option costs that kernel plus the copy of the two buffers."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import B_LOCAL, HORIZON, NUM_STEPS, build_model          # noqa: E402
from dreamer4_amd.learner import run_learner                       # noqa: E402

VARIANTS = (('off', False, False), ('keep_reward_ema_stats', True, False), ('clip_values', False, True), ('both', True, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'learn_norm_cost.txt'))
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--inner', type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('learn_norm_cost needs the GPU: a CPU has no learner to time')
    dev = torch.device('cuda:0')
    m = build_model(dev)
    dreams = m.generate(HORIZON + 1, batch_size=B_LOCAL, num_steps=NUM_STEPS, return_rewards_per_frame=True, return_agent_actions=True,
                        return_log_probs_and_values=True)

    def step(ema, clip):
        m.keep_reward_ema_stats, m.clip_values = ema, clip
        return run_learner(m, dreams, 'ppo')[0]

    losses = {}
    for name, ema, clip in VARIANTS:                                  # warm-up of every variant (workspace, tile choices, code objects)
        for _ in range(3):
            losses[name] = step(ema, clip)
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in VARIANTS}
    for r in range(a.rounds):
        order = VARIANTS[r % 4:] + VARIANTS[:r % 4]
        for name, ema, clip in order:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.inner):
                step(ema, clip)
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / a.inner)
    base = statistics.median(times['off'])
    lines = [f'learner step (d4_learn: losses + gradients of both heads), cfg 2 heads, B = {B_LOCAL}, T = {HORIZON + 1} ({B_LOCAL * (HORIZON + 1)} rows), ppo, fp32',
             f'{torch.cuda.get_device_name(0)}; device events around {a.inner} steps, {a.rounds} rounds, the four variants alternating within a round',
             f"{'variant':<24}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'vs off (median)':>17}"]
    for name, _, _ in VARIANTS:
        t = times[name]
        med = statistics.median(t)
        lines.append(f'{name:<24}{med:>11.4f}{min(t):>9.4f}{max(t):>9.4f}{1e3 * (med - base):>+14.1f} us')
    lines.append('losses [policy, value]: ' + '; '.join(f'{k} {[round(x, 6) for x in v.tolist()]}' for k, v in losses.items()))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
