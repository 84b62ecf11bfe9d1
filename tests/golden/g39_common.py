"""Shared by the G39 fixture generator and the PathNet trainer tests: the scripted runs (settings, schedule, seeds)."""
N, M, L = 2, 4, 8                        # the tiny net of g38_common, setting "a"
GENERATIONS, NEPOCHS = 3, 6              # 2 epochs per participant per generation
LR, LR_FACTOR, LR_PATIENCE = 0.05, 2, 4  # a short patience, so that the LR division is reached
PHASE1_EPOCHS = 12
SEEDS = {"joint_t0": 390, "joint_t1": 391, "phase1_t0": 392, "phase1_t1": 393}
