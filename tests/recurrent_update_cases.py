"""The shapes at which test_gpu_recurrent_distill.py and test_gpu_recurrent_ppo.py hold one update of SequenceLearner / SequencePPOLearner to fp64, shared
so that both learners meet the same ones.  A helper module like learn_cases.py; it needs no GPU.

    id        T   N  B_env   R   rows   what it is for
    small     3   9    5    16     15   the shape both tests had before: every split-K factor is 1 (rows // 16 == 0)
    shipped  20  60   51    64   1020   what distill.py / train_finetune.py run and DESIGN.md 24 / 25 time: S = 63 five times, 24, 32, and 63 does not
                                        divide 1020 (uneven split-K chunks); 20 steps of backward recurrence over 51-row products
    wide     20  16   13   256    260   the largest memory: three 64-column tiles of W_hh per gate block, S up to 16
    one_step  1  80   70    48     70   no recurrence at all, every env cleared: m0 = 0 everywhere, so W_hh's gradient is exactly 0
    cut       2  40   33    80     66   every env cleared at the last step: nothing comes back through the memory
    single   20   4    1    64     20   one env: 1-row products at every step, a clear in the middle, every S = 1

The minibatch is a permuted subset of the N envs.  Clears (t, env) for shipped and wide: one env of the minibatch at t = 0, another at t = T - 1 (a clear
in the last row), a third at every t, the rest never; envs outside the minibatch carry clears too, which must not reach it.
"""
import torch

CASES = {"small": (3, 9, 5, 16), "shipped": (20, 60, 51, 64), "wide": (20, 16, 13, 256), "one_step": (1, 80, 70, 48), "cut": (2, 40, 33, 80),
         "single": (20, 4, 1, 64)}
IDS = list(CASES)


def minibatch(name):
    """-> (T, N, B_env, R, envs [B_env] as a list, clears [(t, env)])"""
    T, N, B, R = CASES[name]
    if name == "small":
        return T, N, B, R, [7, 0, 3, 8, 2], [(1, 0), (1, 8), (2, 4)]                # envs 0 and 8 are in the minibatch, env 4 is not
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(100 * T + N)).tolist()
    envs, rest = perm[:B], perm[B:]
    if name in ("shipped", "wide"):
        clears = [(0, envs[0]), (T - 1, envs[1])] + [(t, envs[2]) for t in range(T)] + [(1, rest[0]), (T // 2, rest[0]), (T - 1, rest[1])]
    elif name == "one_step":
        clears = [(0, e) for e in range(N)]
    elif name == "cut":
        clears = [(1, e) for e in range(N)]
    else:
        clears = [(7, envs[0])]
    return T, N, B, R, envs, clears


def clears_inside(envs, clears):
    """the number of clear flags that fall on the minibatch's envs"""
    return len({(t, e) for t, e in clears if e in envs})


def check_split_k(name, S):
    """the conditions that keep a case from quietly degrading: S is the learner's list of split-K factors of its seven weight gradients"""
    T, _, B, _ = CASES[name]
    assert len(S) == 7
    if name in ("small", "single"):
        assert S == [1] * 7, S
    else:
        assert max(S) > 1, S
    if name == "shipped":
        assert T * B == 1020 and 63 in S and 1020 % 63 != 0 and S == [63, 63, 63, 63, 63, 24, 32], S
