"""Constants and data shared by the G37 generator (reference run, dev container) and the iCaRL tests: g35_common's small
BN-free net on 3x16x16 inputs, three 4-class tasks on one 12-way head, about 24 training images per class.  numpy only."""
import numpy as np

import g35_common as I35

N_TASKS, NC_PER_TASK, N_OUT, HW = 3, [4, 4, 4], 12, 16
N_MEMORIES = 8                    # total 24: K/m = 6 -> 3 -> 2 over the three tasks (truncation twice)
LR, WD, REG = 0.05, 1e-4, 1.5
SEED = 3712
HERD_BATCH = 10                   # the reduced args.batch_size of manage_memory: classes of 22-26 images -> a short last batch
EVAL_BATCH = 10                   # args.batch_size of the evaluation
B, N_APPEND, TOTAL_BATCH = 5, 9, 3   # observe steps of task 3: 5 current rows, 9 exemplars, distillation chunks of 3 (two chunks per task)
STEPS, WARM_STEPS = 3, 12         # recorded steps at task 3; unrecorded steps at task 2 (they move the parameters)
CLASS_SIZES = [[24, 22, 25, 23], [26, 24, 23, 24], [22, 25, 24, 26]]
N_TEST = 7


def make_net():
    return I35.make_net(False)


def task_data(task):
    """(x [n,3,16,16] f32, y [n] i64 in 0..3) of one task's training set, classes interleaved; class-dependent means."""
    gen = np.random.RandomState(SEED + 10 + task)
    y = np.concatenate([np.full(n, c) for c, n in enumerate(CLASS_SIZES[task])])
    y = y[gen.permutation(len(y))]
    x = gen.standard_normal((len(y), 3, HW, HW)).astype(np.float32) + ((y[:, None, None, None] - 1.5) * 0.5 + task * 0.3).astype(np.float32)
    return x.astype(np.float32), y.astype(np.int64)


def step_batches(task, n):
    gen = np.random.RandomState(SEED + 20 + task)
    out = []
    for _ in range(n):
        y = gen.randint(0, 4, B)
        x = gen.standard_normal((B, 3, HW, HW)).astype(np.float32) + ((y[:, None, None, None] - 1.5) * 0.5 + task * 0.3).astype(np.float32)
        out.append((x.astype(np.float32), y.astype(np.int64)))
    return out


def probe_batch():
    gen = np.random.RandomState(SEED + 30)
    return gen.standard_normal((N_TEST, 3, HW, HW)).astype(np.float32)


def seed_draws(task):
    """Seeds of the three host generators in front of the observe steps of a task (generator and replays alike)."""
    import random
    import torch
    torch.manual_seed(SEED + 40 + task)
    random.seed(SEED + 50 + task)
    np.random.seed(SEED + 60 + task)


def constants():
    return dict(N_TASKS=N_TASKS, NC_PER_TASK=NC_PER_TASK, N_OUT=N_OUT, HW=HW, N_MEMORIES=N_MEMORIES, LR=LR, WD=WD, REG=REG, SEED=SEED,
                HERD_BATCH=HERD_BATCH, EVAL_BATCH=EVAL_BATCH, B=B, N_APPEND=N_APPEND, TOTAL_BATCH=TOTAL_BATCH, STEPS=STEPS,
                WARM_STEPS=WARM_STEPS, CLASS_SIZES=CLASS_SIZES)
