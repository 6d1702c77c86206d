"""fp64 reference pieces for the external torso wrench (PgttBuffers.xfrc) - TEST INFRASTRUCTURE, no GPU needed: the env's DR'd model
dict, hold actions, J_torso^T w from mjcf.kinematics_np / jacobians_np, and the minimiser of one substep's convex problem.  Shared by
tests/test_gpu_push.py and tests/test_gpu_wrench_variants.py; tests/test_wrench_reference.py holds torso_wrench_qfrc to facts of its own."""
import numpy as np

from phase_guided_terrain_traversal_amd import abi, mjcf


def _model_for(model, prm):
    """the env's DR'd model dict (body masses, torso COM, hinge zero offsets, armature) for the fp64 helpers of mjcf"""
    m = dict(model)
    m["body_mass"] = prm[abi.P_BODY_MASS:abi.P_BODY_MASS + 13].astype(np.float64)
    ipos = np.array(model["body_ipos"], np.float64).copy(); ipos[0] = prm[abi.P_BASE_IPOS:abi.P_BASE_IPOS + 3]
    m["body_ipos"] = ipos
    q0 = np.array(model["qpos0"], np.float64).copy(); q0[7:] = prm[abi.P_QPOS0:abi.P_QPOS0 + 12]
    m["qpos0"] = q0
    arm = np.array(model["dof_armature"], np.float64).copy(); arm[6:] = prm[abi.P_ARMATURE:abi.P_ARMATURE + 12]
    m["dof_armature"] = arm
    return m


def _hold_action(model, qpos, cfg):
    """actions whose motor targets equal the current hinge angles (no actuator force at zero hinge velocity)"""
    key = np.asarray(model["key_qpos"], np.float32)
    act = np.zeros((qpos.shape[1], 12), np.float32)
    for ac in range(12):
        j = 3 * ((ac // 3) ^ 1) + ac % 3
        act[:, ac] = (qpos[7 + j].astype(np.float32) - key[7 + ac]) / np.float32(cfg["action_scale"])
    return act


def torso_wrench_qfrc(model, qpos, w, at_origin=False):
    """J_p^T f + J_r^T t in fp64 for the wrench w = (world force f, world torque t) on the torso, J at the torso's centre of mass xipos[0]
    (mj_applyFT): what mj_xfrcAccumulate adds to qfrc_smooth.  `model`: the model dict of mjcf.load_model, or the DR'd one of _model_for (its
    body_ipos[0] and qpos0 are the env's).  at_origin: take the arm at the body origin xpos[0] instead of the COM - NOT the wrench the env applies;
    only the resolving-power checks use it (a kernel that forgot base_ipos would compute this)."""
    qpos = np.asarray(qpos, np.float64)
    w = np.asarray(w, np.float64)
    xpos, xquat, xmat, xipos, ximat = mjcf.kinematics_np(model, qpos)
    jp, jr = mjcf.jacobians_np(model, xpos, xmat, xpos[0] if at_origin else xipos[0], 0)
    return jp.T @ w[0:3] + jr.T @ w[3:6]


def _minimiser(D, qfrc_smooth):
    """fp64 minimiser of 1/2 (a - qs)^T M (a - qs) + 1/2 sum_active D_r min(0, J_r a - aref_r)^2 with qs = M^-1 qfrc_smooth (Newton on the active set,
    backtracking on the cost)"""
    M, J, Dd, aref = D["qM"], D["efc_J"], D["efc_D"], D["efc_aref"]
    on = np.asarray(D["efc_active"]) != 0
    qs = np.linalg.solve(M, qfrc_smooth)

    def cost(a):
        r = J @ a - aref
        act = on & (r < 0)
        d = a - qs
        return 0.5 * d @ M @ d + 0.5 * (Dd * r * r * act).sum(), act, r

    a = qs.copy()
    c, act, r = cost(a)
    for _ in range(200):
        H = M + (J[act].T * Dd[act]) @ J[act]
        g = M @ (a - qs) + J[act].T @ (Dd[act] * r[act])
        step = -np.linalg.solve(H, g)
        s = 1.0
        while True:
            c2, act2, r2 = cost(a + s * step)
            if c2 <= c + 1e-14 * abs(c) or s < 1e-10:
                break
            s *= 0.5
        a, c, act, r = a + s * step, c2, act2, r2
        if np.abs(s * step).max() < 1e-13 * (1 + np.abs(a).max()):
            break
    return a
