"""The plumbing of the sampled recurrent actor and of recurrent_ppo.py that needs no GPU: the argument struct of pgtt_learn_recurrent_act_sample
against the header, the exports, FinetuneConfig, the refusals of finetune() and of train_finetune.py, and the file round trip."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from phase_guided_terrain_traversal_amd import learn, ppo, recurrent_ppo  # noqa: E402
from phase_guided_terrain_traversal_amd.policy import PolicyMLP, _DIR as POLICY_DIR  # noqa: E402
from phase_guided_terrain_traversal_amd.recurrent_policy import RecurrentPolicy, SequenceLearner  # noqa: E402

P177 = os.path.join(POLICY_DIR, "policy177.npz")
CTYPES = {"float*": C.c_void_p, "int64_t*": C.c_void_p, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "int32_t": C.c_int32}


def test_the_c_mirror_has_the_headers_fields():
    """field names, order and kinds of PgttLearnRecurrentSampleArgs against include/pgtt_learn.h; its size from the embedded struct's size"""
    text = open(os.path.join(ROOT, "include", "pgtt_learn.h")).read()
    name, mirror = "PgttLearnRecurrentSampleArgs", learn.PgttLearnRecurrentSampleArgs
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            kind, names = decl.replace("const ", "").split(None, 1)
            for f in names.split(","):
                f = f.strip()
                fields.append((f.lstrip("*"), kind + "*" if f.startswith("*") and not kind.endswith("*") else kind))
    assert fields[0] == ("act", "PgttLearnRecurrentActArgs") and mirror._fields_[0] == ("act", learn.PgttLearnRecurrentActArgs)
    assert [f for f, _ in fields] == [f for f, _ in mirror._fields_], fields
    assert [CTYPES[k.replace(" ", "")] for _, k in fields[1:]] == [t for _, t in mirror._fields_[1:]]
    assert C.sizeof(mirror) == C.sizeof(learn.PgttLearnRecurrentActArgs) + 4 * 8 + 8 + 8 + 8 == 296         # the int32 is padded to the struct's alignment
    assert mirror.eps.offset == 240 and mirror.deterministic.offset == 288
    for fn in ("pgtt_learn_recurrent_act_sample", "pgtt_learn_sizeof_recurrent_sample_args"):
        assert fn in learn.EXPORTS and re.search(r"\b" + fn + r"\(", text), fn
    assert learn.SIDE.sizeofs["pgtt_learn_sizeof_recurrent_sample_args"] is mirror
    proto = learn.SIDE.prototypes["pgtt_learn_recurrent_act_sample"]
    assert proto[1][0] is C.POINTER(mirror) and proto[1][1] is C.c_void_p


def test_the_header_states_the_new_entry():
    text = open(os.path.join(ROOT, "include", "pgtt_learn.h")).read()
    for needle in ("softplus_t(raw) + 1e-3f", "0x50475454", "0.91893853320467274f", "0.69314718055994531f", "6.28318530717958648f", "j ascending",
                   "2304 bytes", "Rows past num_envs are neither drawn for nor stored"):
        assert needle in text, needle


def test_finetune_config_is_ppo_config_plus_two():
    cfg = recurrent_ppo.FinetuneConfig()
    base = ppo.PPOConfig()
    assert isinstance(cfg, ppo.PPOConfig) and cfg.critic_warmup_iters == 50 and cfg.iterations == 20 and cfg.learning_rate == 3e-5
    for k in ("unroll_length", "num_minibatches", "num_updates_per_batch", "discounting", "gae_lambda", "entropy_cost", "clipping_epsilon",
              "max_grad_norm", "reward_scaling"):
        assert getattr(cfg, k) == getattr(base, k), k
    assert not hasattr(cfg, "memory")                                                  # the memory's size is the policy's


class _Env:
    def __init__(self, n, device="cpu"):
        self.num_envs, self.device = n, torch.device(device)
        self.observation_size = {"state": 171, "privileged_state": 215}


def test_finetune_refusals():
    pi = RecurrentPolicy.from_teacher(PolicyMLP(P177), 16)
    cfg = recurrent_ppo.FinetuneConfig(num_minibatches=4)
    with pytest.raises(recurrent_ppo.FinetuneError, match="does not divide"):
        recurrent_ppo.finetune(_Env(10), pi, cfg)
    with pytest.raises(recurrent_ppo.FinetuneError, match="GPU only"):
        recurrent_ppo.finetune(_Env(8), pi, cfg)

    class Fake:
        memory, dims = 24, (171, 512, 256, 128, 24)
    with pytest.raises(recurrent_ppo.FinetuneError, match="multiple of 16"):
        recurrent_ppo.finetune(_Env(8), Fake(), cfg)
    env = _Env(8)
    env.curriculum = object()
    with pytest.raises(recurrent_ppo.FinetuneError, match="GPU only|curriculum"):
        recurrent_ppo.finetune(env, pi, cfg)
    with pytest.raises(learn.LearnError, match="GPU only"):                             # the learner itself has no CPU form either
        z = torch.zeros
        recurrent_ppo.SequencePPOLearner(recurrent_ppo.RecurrentActorCritic(pi, 215), None, z(2, 3, 171), z(2, 3, 12), z(2, 3), z(2, 3, 16),
                                         z(2, 3, dtype=torch.uint8), z(2, 3, 215), z(2, 3), z(2, 3), z(215), torch.ones(215), 3, cfg)
    assert issubclass(recurrent_ppo.SequencePPOLearner, SequenceLearner)


def test_the_actor_critic_walks_the_policy_first():
    pi = RecurrentPolicy.from_teacher(PolicyMLP(P177), 16)
    model = recurrent_ppo.RecurrentActorCritic(pi, 215)
    params = list(model.parameters())
    assert len(params) == 13 + 8 and {id(p) for p in params[:13]} == {id(t) for t in pi.tensors()}      # the policy's thirteen, in the module's own order
    lins = [m for m in model.value if isinstance(m, torch.nn.Linear)]
    assert [(l.in_features, l.out_features) for l in lins] == [(215, 512), (512, 256), (256, 128), (128, 1)]
    flat = learn.FlatParams(model)                                                     # CPU tensors: the aliasing needs no GPU
    assert flat.offset_of[id(lins[0].weight)] == sum(p.numel() for p in pi.tensors())
    assert all(flat.offset_of[id(t)] < flat.offset_of[id(lins[0].weight)] for t in pi.tensors())
    w0 = pi.layers[0].weight
    assert flat.grad_of(w0).data_ptr() == flat.grad.data_ptr() + 4 * flat.offset_of[id(w0)] and w0.data_ptr() == flat.flat.data_ptr() + 4 * flat.offset_of[id(w0)]


def test_train_finetune_parser_and_refusals(tmp_path):
    import train_finetune as tf
    ap = tf.make_parser()
    with pytest.raises(SystemExit):
        ap.parse_args([])                                                              # --policy is required
    a = ap.parse_args(["--policy", "policy177"])
    assert (a.terrain, a.obs, a.num_envs, a.num_minibatches, a.critic_warmup, a.memory, a.iters, a.max_seconds) == ("level4", "elevation", 4096, 32, 50, 64, 20, 0.0)
    assert a.learning_rate == recurrent_ppo.FinetuneConfig().learning_rate
    for obs in ("elevation", "elevation_filled", "student", "state"):
        assert ap.parse_args(["--policy", "x", "--obs", obs]).obs == obs
    with pytest.raises(SystemExit):
        ap.parse_args(["--policy", "x", "--obs", "depth"])
    a = ap.parse_args(["--policy", "policy177", "--terrain", "level10", "--elevation", "--critic_warmup", "3", "--max_seconds", "120", "--iters", "7"])
    assert a.elevation is not None and a.critic_warmup == 3 and a.max_seconds == 120.0
    cfg = tf.make_config(a)
    assert (cfg.critic_warmup_iters, cfg.iterations, cfg.unroll_length, cfg.num_minibatches, cfg.num_updates_per_batch) == (3, 7, 20, 32, 4)
    with pytest.raises(SystemExit, match="does not divide"):
        tf.check_args(ap.parse_args(["--policy", "x", "--num_envs", "100", "--num_minibatches", "32"]), device="cuda:0")
    with pytest.raises(SystemExit, match="GPU only"):
        tf.check_args(ap.parse_args(["--policy", "x"]), device="cpu")
    # a feed-forward file gets a memory with a zero read-out; a memory that is no multiple of 16 is refused; a recurrent file keeps its own
    pi = tf.load_policy("policy177", 32)
    assert pi.memory == 32 and bool((pi.mem_w == 0).all()) and torch.equal(pi.layers[0].weight, PolicyMLP(P177).layers[0].weight)
    for bad in (0, 24, 272):
        with pytest.raises(SystemExit, match="multiple of 16"):
            tf.load_policy("policy177", bad)
    with pytest.raises(SystemExit, match="no such file"):
        tf.load_policy("no_such_policy", 16)
    path = str(tmp_path / "recurrent.npz")
    with torch.no_grad():
        pi.mem_w.copy_(torch.randn(24, 32) * 0.1)
    pi.save(path)
    back = tf.load_policy(path, 64)
    assert back.memory == 32 and all(torch.equal(x, y) for x, y in zip(pi.tensors(), back.tensors()))


def test_the_file_round_trip(tmp_path):
    """Finetuned.save writes the 13-tensor file of RecurrentPolicy.save: equal bits through RecurrentPolicy.load, read by the evaluator's switch"""
    import evaluate
    pi = RecurrentPolicy.from_teacher(PolicyMLP(P177), 16, seed=5)
    with torch.no_grad():
        pi.mem_w.copy_(torch.randn(24, 16) * 0.1)
    model = recurrent_ppo.RecurrentActorCritic(pi, 215)
    learn.FlatParams(model)                                                            # the parameters are views of the flat buffer from here on
    out = recurrent_ppo.Finetuned(model, [], None)
    path = str(tmp_path / "finetuned.npz")
    out.save(path)
    back = RecurrentPolicy.load(path)
    assert all(torch.equal(x, y) for x, y in zip(pi.tensors(), back.tensors())) and torch.equal(pi.mean, back.mean) and torch.equal(pi.std, back.std)
    assert len(np.load(path).files) == 15 and evaluate.recurrent_file(path)
