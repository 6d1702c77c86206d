/*
 * pgtt_elevation.h — C ABI of libpgtt_elevation.so: a depth-fused elevation map per env, and the 13 x 9 height scan sampled from it.
 *
 * The geometric counterpart of the student (pgtt_perceive.h): the onboard depth image (pgtt_depth.h) is unprojected with the camera pose, fused
 * into a rolling robot-centred map of world heights, and the observation's 117 scan rows are read from the map.  Nothing is learned.
 * A separate library from libpgtt.so and the other side libraries: it only READS the env's `state`, `obs` and `done` and the camera's image, and
 * writes the caller's `map`, `origin`, `est`, `known` and `obs_out`.
 *
 * Conventions (those of pgtt.h)
 *   - plain C; `stream` is a hipStream_t passed as void*.
 *   - every function returns 0 or a negative PGTT_E_* code (pgtt.h); the message is available from pgtt_elevation_last_error().
 *   - device buffers are CALLER-OWNED; pgtt_elevation() enqueues ONE kernel on the caller's stream and neither allocates, synchronises nor
 *     reads anything back, so it can be captured in a HIP graph.  The library reads no environment variable.
 *   - everything is fp32 on the device, and the order of the steps below is fixed.
 *
 * Camera.  The camera model of pgtt_depth.h: width, height, fovy_deg, near, far, mount_pos, mount_quat; optical axis fwd = the camera frame's +x,
 * up = its +z, right = fwd x up; pixel (i, j) (row i from the top, column j) is sampled at its centre,
 *     u = (2 (j + 0.5) / W - 1) * tan(fovy / 2) * W / H,   v = (1 - 2 (i + 0.5) / H) * tan(fovy / 2).
 * Only a camera on the torso is supported (mount_body == 0, anything else is PGTT_E_ARG), so no forward kinematics is needed:
 *     camera pose = base pose * mount pose,   base pose = rows PGTT_S_QPOS + 0..6 of `state`, the quaternion normalised first.
 * mount_quat is normalised by pgtt_elevation_create.  The image is taken as the pose's own: a caller whose sensor period is above 1 would
 * unproject a stale image under a moved pose, and must not call pgtt_elevation() or pgtt_elevation_points() on the steps its sensor skips - such
 * a caller uses pgtt_elevation_follow() ("Following a slower sensor" below).
 *
 * Map.  Per env, map[G][G] (G = cfg.grid) holds world-z heights in metres; NaN = unknown.  The window is world-aligned and toroidal, with
 * square cells of side `res`:
 *     world cell (ix, iy) = (floor(x / res), floor(y / res)) lives at slot map[ix mod G][iy mod G]    (floor-mod: negative coordinates work)
 *     origin[e] = (floor(bx / res), floor(by / res)), the cell of the base position (bx, by), is the window's centre cell
 *     the window holds the cells [origin - G/2, origin - G/2 + G) per axis (G/2 rounded down)
 * Limits: 8 <= G <= 96 (PGTT_ELEVATION_MIN_GRID / MAX_GRID; 4 G G <= 36864 bytes of LDS), res > 0.
 * Before the first call the caller fills `map` with NaN, or passes clear_all to the first call; `origin` may hold anything then.
 *
 * One pgtt_elevation() call does, per env, in this order:
 *  1. Clear.  Every cell becomes NaN when clear_all != 0, or clear_mask[e] != 0, or use_done != 0 and done[e] != 0.  A cleared env takes the new
 *     origin directly.
 *  2. Recentre.  The new origin is computed from the current base position.  Every slot whose world cell under the new window differs from its
 *     world cell under the old window (origin[e] as the last call left it) becomes NaN; a jump of G cells or more clears everything.
 *     origin[e] is written.
 *  3. Tick maximum.  For every pixel with near < d < far (a NaN, a miss that reads `far` and a dropout pixel are all skipped):
 *         p = cam_pos + R_cam (d, d u, d v) in (fwd, right, up): the depth is the distance along the optical axis
 *         skipped when p, expressed in the base frame, lies in the box |x| <= self_half[0], |y| <= self_half[1], |z| <= self_half[2] - the self
 *           filter of a camera that sees the robot (see_robot); self_half = (0, 0, 0) disables it
 *         skipped when p's cell is outside the window
 *         otherwise m[cell] = max(m[cell], p.z)
 *     m lives in LDS and is updated with an LDS atomic maximum (on an order-preserving integer key of the fp32 value): the result does not
 *     depend on the order of the lanes, so the map is deterministic.
 *  4. Fuse.  For the cells step 3 touched: h = isnan(h) ? m : h + alpha (m - h), alpha in (0, 1]; alpha = 1 replaces the old value (by m itself,
 *     bit for bit).
 *  5. Sample.  The scan grid of the observe kernel, point i = 9 r + c: ox = (6 - r) scan_dist_x, oy = (4 - c) scan_dist_y, rotated by
 *         yaw = atan2(2 (qw qz + qx qy), 1 - 2 (qy^2 + qz^2))      of the normalised base quaternion
 *     and offset from the base xy.  z[i] = the value of the cell that contains the point; known[i] = 1 when that cell is inside the window and
 *     not NaN, else 0.  An unknown point takes the minimum over the known points; when no point is known every z is 0.  Then
 *         est[i] = z[i] - min z:    the observation's noise-free scan rows (heights above the lowest scan point), 0 at an unknown point.
 *  6. Assemble.  When obs_out is bound: obs_out = obs with rows [scan_row0, scan_row0 + 117) replaced by est, every other row copied bit for
 *     bit (scan_row0 = 38 for the PGTT task, 30 for the baseline).
 *
 * An env's outputs are functions of its own rows only: the same bits at any batch position and at any N.
 *
 * use_done and auto-reset.  With PgttConfig.autoreset = 1 the step that finishes an episode leaves done[e] = 1 AND has already restored the
 * env's qpos rows to the new episode's first state, so a call with use_done after the step clears the map and integrates the first image of the
 * new episode under its own pose.  With autoreset = 0 the state rows stay the finished episode's and done[e] stays as the step's termination
 * test gives it: use_done then clears the map at every call while done[e] != 0, so it holds that call's image alone, until the caller resets the
 * env (pgtt_reset with a mask) and passes the same mask as clear_mask.
 *
 * A point cloud in place of the image.  pgtt_elevation_bind_points() binds, next to the buffers, `points`: device [N][P][3], WORLD points, P >= 1
 * (the points of pgtt_lidar.h, registered at the pose they were taken from; any other source of world points will do).  pgtt_elevation_points()
 * then runs the six steps above in the same order with step 3 replaced - for every point k < P of the env:
 *         skipped when one of its coordinates is NaN or not finite (a ray without a return)
 *         skipped inside the self-filter box (the test of step 3, on the point itself)
 *         skipped when its cell is outside the window
 *         otherwise m[cell] = max(m[cell], p.z), with the same LDS atomic on the order-preserving key
 * The camera fields of the config (width .. mount_quat) are not read by it; they must still be valid for pgtt_elevation_create.
 * Both sources may feed one handle: bound by pgtt_elevation_bind_points with a depth image too, pgtt_elevation() is what it is on a handle bound
 * by pgtt_elevation_bind.
 *
 * Hole filling.  pgtt_elevation_fill() is a launch of its own behind a tick.  It READS what the tick left - `map`, `origin`, `state` and `obs` as
 * they are bound - and writes only the outputs of PgttElevationFill: never `map`, `origin`, `est`, `known` or the tick's `obs_out`.  A filled height
 * is a hypothesis (what a sensor cannot see is usually lower than what it can): it is never fused, and the next tick does not see it.
 * Per env, with lo = origin - G/2: the window cell (a, b), 0 <= a, b < G, is world cell (lo_x + a, lo_y + b), stored at slot
 * ((lo_x + a) mod G, (lo_y + b) mod G) as above.
 *   Start.   D(a, b) = 0 where the cell is not NaN, else 255; W = the map.
 *   Pass p = 1 .. passes.  Every cell that still has D = 255 looks at its up to eight neighbours (a +- 1, b +- 1) INSIDE THE WINDOW - the window's
 *            edges are edges; the toroidal storage does not connect the far sides - and of them at those that were known at the end of pass
 *            p - 1 (D < p).  If there is one: W = the minimum of their values, D = p.  A cell filled in pass p is not a source in pass p (a Jacobi
 *            pass), so the result does not depend on the order of the lanes, and D is the Chebyshev distance inside the window to the nearest
 *            measured cell, for distances up to `passes`.
 *   Minimum. In the total order of the tick maximum's integer key: -0 < +0, the infinities are ordinary values, and the result is one of the inputs
 *            bit for bit.
 *   Stopping after a pass that filled nothing has no visible effect, and is done.  1 <= passes <= PGTT_ELEVATION_MAX_GRID - 1: more cannot fill
 *            anything in a window of 96 cells, and D fits a byte with 255 free.
 *   Sample.  Step 5 on the filled window: z[i], dist[i] = W, D of the cell that contains scan point i; dist[i] = 255 outside the window or where the
 *            cell is still unknown.  A point with dist = 255 takes the minimum (in the key's order) over the others; every z is 0 when there are
 *            none.  est[i] = z[i] - min z.
 *   Assemble.  Step 6 into the fill's own obs_out.
 *   Dense.   map_out is W and dist_out is D, both in the map's slot layout; a cell that is still unknown is NaN.
 * An origin outside +-2^30 (a map never ticked) is taken as +-2^30.  One launch, one workgroup per env, W and D of the window and a border of one cell in LDS: 5 (G + 2)^2 bytes.
 *
 * Following a slower sensor.  A sensor of period `every` > 1 (PgttDepthConfig.every, PgttLidarConfig.every) recomputes its image or points at one
 * call in `every` and decides that on the device, from its counter.  A tick on the other steps would unproject a stale image under a moved pose, or
 * fuse a stale point cloud once more, which for alpha < 1 weights it again.  pgtt_elevation_follow() is the call for such a sensor: it fuses when
 * the sensor has new data and, in between, leaves the map alone and answers the height queries at the current pose - what a robot's mapping stack
 * does.  pgtt_elevation_bind_rate() hands it the SENSOR's device counter and period; it is called BEHIND the sensor's call of the same step, with the
 * `force` that call was given.  With c = counter[0] - 1, the counter's value before the sensor's call (which has advanced it by one), the call is
 *     fresh   when force != 0, or c >= 0 and c mod every == 0: the sensor's own rule, evaluated on the device,
 *     a hold  otherwise.
 * There is no read-back, no synchronisation and no allocation: at most two launches on `stream`, of which one returns at once in every workgroup,
 * so the step stays one capturable sequence.
 *   Fresh call.  The six steps of pgtt_elevation() - or of pgtt_elevation_points(), by which bind was made last - in the same order; every output
 *            has the same bits.
 *   Hold call.   Per env:
 *     1. Clear.  The rule of step 1: clear_all, clear_mask[e], or use_done and done[e] != 0.  A cleared env's whole map becomes NaN and its
 *        origin[e] the cell of its current base position.
 *     2. Nothing else is written: the `map` and `origin` of an env that is not cleared are not touched.  No recentring, no fusion.
 *     3. Sample.  Step 5 at the CURRENT pose, from the window that origin[e] describes: the origin just written for a cleared env, otherwise the
 *        origin as the last fresh call left it (one outside +-2^30 is taken as +-2^30, as pgtt_elevation_fill does).  A scan point whose cell has
 *        left that window is unknown.  known, the minimum over the known points and est = z - min z are those of step 5; all 0 when nothing is
 *        known.
 *     4. Assemble.  Step 6 into obs_out.
 * An env's outputs depend on its own rows only.  pgtt_elevation_fill() is what it was: it reads `map`, `origin` and `state` as they stand, so behind
 * a hold call it fills and samples the held window at the current pose.  Not covered: an image fused later than it was taken (that needs the pose
 * of its capture; "Sensor latency" below does that for a sensor of period 1), sensor phases per env.
 *
 * Variance-weighted fusion: a Kalman layer.  Steps 3 and 4 above suit noise-free data: the maximum of n noisy samples is biased upwards, and alpha
 * is one gain for every distance.  pgtt_elevation_var() and pgtt_elevation_var_points() are ticks that keep, next to `map`, a second persistent
 * layer `var`: device [N][G][G] fp32 in the slot layout of `map`, the variance of each height in m^2, NaN exactly where `map` is NaN; and that write
 * one more output per tick, est_var [N][117].  The settings, the two buffers and their ranges are PgttElevationVar's (pgtt_elevation_bind_var).  Per
 * env, in this order; `alpha` is not read:
 *  1. Clear.     Step 1 above, on `map` and `var` together.
 *  2. Recentre.  Step 2 above, on `map` and `var` together.
 *  3. Tick maximum.  Step 3 above for the image (pgtt_elevation_var) or for the points (pgtt_elevation_var_points), unchanged: validity,
 *     unprojection, self filter, window test, and zmax[cell] by the LDS atomic maximum on the order-preserving key.
 *  4. Band sums.  A second pass over the same pixels or points.  A pixel that step 3 admitted into `cell` contributes when zmax[cell] - z <= band,
 *     with q = rint((zmax[cell] - z) * 2^18), an integer (PGTT_ELEVATION_BAND_SCALE).  Per cell n = the number of contributors and S = the sum of
 *     their q; the pixel that is the maximum always contributes, with q = 0.  Both are integer sums (LDS integer atomics): the result does not
 *     depend on the order of the lanes, or of the points in `points`.
 *  5. Measurement, per touched cell.
 *         m    = zmax - (S / n) * 2^-18:   the mean of the upper-surface band; with n = 1, m is zmax bit for bit
 *         rho2 = (cx - bx)^2 + (cy - by)^2 + (m - bz)^2,   (cx, cy) = ((ix + 0.5) res, (iy + 0.5) res) the centre of the world cell, b the BASE
 *                position - for both sources: the points call knows no sensor mount, and these are settings, not facts about a sensor
 *         r    = (sigma0^2 + sigma_rel^2 rho2) / min(n, max_count)
 *  6. Predict.  Every cell that is not NaN, touched or not: v = min(v + process, var_max).
 *  7. Update, per touched cell.
 *         the cell is NaN:                     h = m, v = min(r, var_max)
 *         (m - h)^2 <= gate^2 (v + r):         k = v / (v + r), h += k (m - h), v = v r / (v + r)
 *         the gate fails and m > h:            h = m, v = min(r, var_max): the map is an upper-surface map, as the maximum made it
 *         the gate fails and m < h:            the measurement is ignored.  With process > 0 the cell's variance grows tick by tick until a
 *                                              persistent lower measurement passes the gate; with process = 0 it never does.
 *  8. Sample.   Step 5 above on `map`: est and known as there.  est_var[i] = v of the cell that contains scan point i, var_max at an unknown point.
 *  9. Assemble. Step 6 above.
 * An env's outputs depend on its own rows only.  One launch, one workgroup of 256 lanes per env; LDS holds a key word and a 64-bit (n, S) word per
 * slot, 12 G G bytes, and this entry keeps that under the 64 KB a launch gets without an attribute: G <= PGTT_ELEVATION_VAR_MAX_GRID = 64;
 * pgtt_elevation_bind_var refuses a handle with a larger grid (PGTT_E_ARG).
 * pgtt_elevation_fill() is unchanged: it reads `map` as it stands, so it works behind a variance tick; filled cells have no variance.
 * `var` is maintained by these two calls alone, and a caller uses ONE kind of tick on a handle: pgtt_elevation(), pgtt_elevation_points() and
 * pgtt_elevation_follow() on a handle with a variance bound do what they always did and leave `var` stale.
 *
 * Odometry drift: the map on an estimated pose.  Everything above registers the image or the points with the simulator's exact base pose.  A robot
 * dead-reckons its pose from leg odometry and a gyro, and the estimate walks away from the truth in x, y and yaw.  pgtt_elevation_odometry() writes
 * such an estimate, pose_est [7][N], and - when points are bound - the world points re-registered at it, points_est [N][P][3].  A promise makes them
 * usable: EVERY entry of this library reads rows PGTT_S_QPOS + 0..6 of `state` (PGTT_S_QPOS is 0) and no other row, so a [7][N] buffer is a legal
 * `state` for pgtt_elevation_bind, pgtt_elevation_bind_points and all the calls behind them.  The caller binds PgttElevationBuffers.state = pose_est
 * and points = points_est itself; the odometry call uses the handle for N and the device only and neither reads nor rebinds the handle's buffers.
 * The model is an error-state dead reckoning, per env, in fp32, in the fixed order below; in the error-state form all-zero settings return the true
 * pose BY VALUE (x + 0), which a re-integration of increments would not.  The settings (PgttElevationOdometry) are settings, not facts about a robot.
 * Persistent per env is odo[e][PGTT_ELEVATION_ODO_WORDS = 12]:
 *     0..2  e_x, e_y, e_z            the position error, metres
 *     3     psi                      the yaw error, radians, not wrapped
 *     4..6  prev_x, prev_y, prev_z   the TRUE base position at the last call
 *     7, 8  scale_e, bias_e          the episode's odometry scale error and gyro bias (rad/s), drawn once per episode
 *     9..11 reserved, written as 0
 * With b = rows 0..2 and q = rows 3..6 of the true `state` (q raw, not normalised), gid = env_id_offset + e, c = counter[0] as it stands before the
 * call, and u_k = the top 24 bits of word k of a Philox block times 2^-24 (the convention of pgtt_depth.h; key = (seed lo, seed hi)):
 *  Clear.  An env is cleared when clear_all != 0, or clear_mask[e] != 0, or use_done != 0 and done[e] != 0 - the map's own rule; a NULL done clears
 *     nothing.  e = 0, psi = 0, prev = b; with the block (gid, (uint32) c, PGTT_RS_ODOMETRY, 1):
 *         scale_e = scale (2 u_0 - 1),   bias_e = yaw_bias (2 u_1 - 1).
 *     No step is made on this call.
 *  Step (an env that is not cleared).  D = b - prev, L = sqrtf(Dx^2 + Dy^2 + Dz^2); with the block (gid, (uint32) c, PGTT_RS_ODOMETRY, 0):
 *         (n_x, n_y)   = sqrtf(-2 logf(1 - u_0)) * (cos, sin)(2 pi u_1),    (n_z, n_psi) the same on (u_2, u_3)
 *         D'   = (1 + scale_e) D
 *         e_x += (cos psi D'x - sin psi D'y) - Dx + sigma_xy sqrtf(L) n_x          with the OLD psi
 *         e_y += (sin psi D'x + cos psi D'y) - Dy + sigma_xy sqrtf(L) n_y
 *         e_z += (D'z - Dz) + sigma_z sqrtf(L) n_z
 *         psi += bias_e dt + sigma_yaw sqrtf(dt) n_psi,    prev = b
 *     Position noise grows with the distance walked (sigma_xy, sigma_z in m / sqrt(m)), yaw noise with time (sigma_yaw in rad / sqrt(s), yaw_bias in
 *     rad / s).  Roll and pitch stay true: gravity is observable.  The cosine and sine of 2 pi u are taken of the exact product (the half-turn
 *     forms, on 2 u), so the draw carries no rounding of the angle.
 *  Outputs.  pose_est[0..2][e] = b + e;  pose_est[3..6][e] = qz(psi) (x) q, the quaternion product with qz(psi) = (cos psi/2, 0, 0, sin psi/2), not
 *     normalised - the map normalises, as it does for `state`.
 *  Points.  When points are bound, for every k < P, with p the world point and r = p - b:
 *         points_est = p + ((Rz(psi) r) - r) + e              with the NEW psi and e
 *     which is T_est o T_true^-1, written so that zero error returns p by value.  A point with a coordinate that is not finite is written as
 *     three NaNs.
 *  counter[0] advances by one per call, in a launch of its own behind the update: no workgroup reads a counter another has advanced.
 * An env's outputs depend on its own rows and its global id only: the same bits at any batch position, at any N, with or without points.
 * Not covered: loop closure or any correction of the drift, roll or pitch error, drift on the proprioceptive rows of the observation.
 *
 * Visibility clean-up.  The ticks above only ever add heights: a cell keeps what was fused into it until the window leaves it or a later measurement
 * lands in it.  Under a drifting pose a stair edge fused some centimetres ago stays as a ghost next to the real one.  pgtt_elevation_visibility() is
 * a launch of its own, called behind the sensor's call (and behind pgtt_elevation_odometry where that is used) and BEFORE the tick of the same step,
 * with the clear arguments that tick will be given.  A ray that reached its end point while passing below a cell's recorded height contradicts that
 * cell, and the cell is forgotten (NaN).  The source is the image or the points, by which bind was made last.  It reads rows PGTT_S_QPOS + 0..6 of
 * `state` and no other, so the promise of the odometry block holds.  The settings and outputs are PgttElevationVisibility's.  Per env, in fp32, in
 * this order:
 *  1. Skip.  An env the tick behind this call will clear (clear_all != 0, or clear_mask[e] != 0, or use_done != 0 and done[e] != 0) is not looked
 *     at: cleared[e] = 0 and its bound_out is NaN everywhere.  The window is the one origin[e] describes, as the last tick left it; an origin outside
 *     +-2^30 is taken as +-2^30, as pgtt_elevation_fill does.  There is no recentring and `origin` is not written.
 *  2. Rays.  The sensor position s: for the image the camera position of the tick (base + R_base mount_pos); for the points base + R_base sensor_pos.
 *     The end point p: the unprojected pixel of step 3 of the tick (near < d < far, the same formula) or the world point.  A ray whose p the tick
 *     would drop for validity (NaN, not finite, outside near .. far) or by the self filter is not cast; a p outside the window is fine, the ray still
 *     crosses the window.  Only the pixels with i mod stride == 0 and j mod stride == 0, or the points with k mod stride == 0, cast a ray.
 *  3. Samples.  With Lh = hypot(px - sx, py - sy), sample k = 0, 1, ... lies at the horizontal distance r_k = (k + 0.5) res from s:
 *         (x_k, y_k) = (sx, sy) + r_k (px - sx, py - sy) / Lh,      z_k = sz + (pz - sz) r_k / Lh
 *     A sample is made while r_k <= Lh - end_guard and k < 2 G.  Lh == 0, or Lh - end_guard below the first sample, gives no samples and no division
 *     (one reciprocal of Lh per ray otherwise).  The cell of a sample is (floor(x_k * (1 / res)), floor(y_k * (1 / res))) with the reciprocal formed
 *     once, in fp32 - NOT the tick's floor(x / res): a sample within a rounding error of a cell border may fall on the other side of it than the
 *     tick would put it.  The indices are clamped to +-1e9 before the window test, as in the tick, so no coordinate can index outside the map.  A
 *     sample whose cell is outside the window, or whose z_k is NaN, is dropped; otherwise bound[cell] = min(bound[cell], z_k), an LDS atomic minimum
 *     on the tick's order-preserving integer key: the result does not depend on the order of the lanes, pixels or points.  This is a definition
 *     by sampling, not a cell traversal: a ray may clip a cell's corner without sampling it, which errs on the side of keeping cells.
 *  4. Clean.  For every slot with a bound whose height h is not NaN: without a variance layer the cell becomes NaN when h > bound + margin; with
 *     one bound (pgtt_elevation_bind_var) the test is h - sigmas * sqrtf(v) > bound + margin and `var` becomes NaN with `map`.  cleared[e] = the
 *     number of such cells, an integer sum.  bound_out, when bound, is the bound layer in the slot layout of `map`, NaN where no sample fell.
 *  5. Nothing else is written: est, known, obs_out and origin are the tick's outputs and stay as they were.  The tick that follows sees the
 *     cleaned map and does what it always did.
 * An env's outputs depend on its own rows only.  One launch, one workgroup of 256 lanes per env, one key word per slot in LDS (4 G G bytes, every
 * G the map allows), LDS integer atomics only, no global atomics.  Not covered: a hold step behind pgtt_elevation_follow (a stale image must not
 * clean), lowering a cell instead of forgetting it, the rays of pixels that hit nothing.
 *
 * Sensor latency: capture-stamped fusion.  Every tick above unprojects the image under the pose of the same call.  A real depth camera or LiDAR delivers
 * its frame some calls after the shutter; a mapping stack fuses that frame under the pose it had at CAPTURE and answers the height queries at the pose
 * it has now.  pgtt_elevation_delayed() is the tick of a handle with a PgttElevationLatency bound (pgtt_elevation_bind_latency): a ring of D frames
 * and of the poses they were taken at lives on the device, and every env fuses the frame of lat[e] calls ago.  The source is the image or the points,
 * by which bind was made last.  The latency is fixed (lat_lo == lat_hi) or drawn per env per episode in [lat_lo, lat_hi].  With c = counter[0] as it
 * stands before the call and gid = env_id_offset + e, per env, in this order:
 *  1. Clear rule.  The tick's own: clear_all != 0, or clear_mask[e] != 0, or use_done != 0 and done[e] != 0.  A cleared env draws its latency, on
 *     integers alone:   lat[e] = lat_lo + (int) (((uint64) w0 * (uint64) (lat_hi - lat_lo + 1)) >> 32),
 *     w0 = word 0 of the Philox block (gid, (uint32) c, PGTT_RS_LATENCY, 0) under the key (seed lo, seed hi); and its age[e] becomes 0.
 *  2. Push.  Slot w = c mod D (floor-mod on the 64-bit counter): ring_data[w][e] takes the env's current image (or its P points) bit for bit,
 *     ring_pose[w][0..6][e] rows 0..6 of the bound `state`, raw, and age[e] = min(age[e] + 1, D).  No other slot and no other env's part of slot w
 *     is written.
 *  3. Pick.  With L = lat[e]: when L < age[e] the frame is that of slot (c - L) mod D (floor-mod) and fused[e] = 1; otherwise the frame that would be
 *     due predates the episode, nothing is fused and fused[e] = 0.
 *  4. Stamped tick.  The six steps of pgtt_elevation() or pgtt_elevation_points() with two poses.  Steps 1, 2, 5 and 6 - clear, recentre and
 *     `origin`, sample, assemble - use the CURRENT pose (the bound `state`).  Step 3 uses the CAPTURE pose from the ring for the camera pose, the basis
 *     of the unprojection and the base position and rotation of the self filter; it takes the frame from the ring and tests the cells against the
 *     NEW window.  Step 4 is unchanged.  Without a frame step 3 admits nothing: the map is cleared or recentred and the scan sampled from what it holds.
 *  counter[0] advances by one per call, in a launch of its own behind the others: no workgroup reads a counter another has advanced.
 * With lat_lo = lat_hi = 0 every output (map, origin, est, known, obs_out) has the bits of the plain tick: the capture pose is a copy of the current
 * rows and the frame a copy of the current image.  An env's outputs, lat included, depend on its own rows and its global id only: the same bits at
 * any batch position and at any N.  The ring stores whatever `state` and `points` the handle is bound to: with odometry those are pose_est and
 * points_est, the map is registered with the estimate the robot had at capture, and nothing in the odometry call changes.  pgtt_elevation_fill()
 * behind it is what it was.  Not covered: the variance tick, visibility and pgtt_elevation_follow behind a latency (a sensor of period 1 is assumed;
 * the Python layer refuses these combinations), sub-step latencies, latency on the proprioceptive rows of the observation.
 */
#ifndef PGTT_ELEVATION_H_
#define PGTT_ELEVATION_H_

#include <stdint.h>

#include "pgtt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGTT_ELEVATION_MAX_DIM 256       /* width and height of the image */
#define PGTT_ELEVATION_MIN_GRID 8
#define PGTT_ELEVATION_MAX_GRID 96       /* 4 * 96 * 96 = 36864 bytes of LDS */

typedef struct PgttElevationConfig {
  int32_t width, height;                 /* 1 .. PGTT_ELEVATION_MAX_DIM each */
  float fovy_deg;                        /* vertical field of view, in (0, 180) */
  float near, far;                       /* 0 < near < far, metres along the optical axis */
  int32_t mount_body;                    /* must be 0 (the torso) */
  float mount_pos[3];                    /* camera pose in the torso frame */
  float mount_quat[4];                   /* wxyz, non-zero; normalised by pgtt_elevation_create */
  int32_t grid;                          /* G: cells per side of the window */
  float res;                             /* cell size in metres, > 0 */
  float alpha;                           /* fusion gain, in (0, 1] */
  float self_half[3];                    /* >= 0: half extents of the self-filter box in the base frame; all 0 = no filter */
  float scan_dist_x, scan_dist_y;        /* PgttConfig.scan_dist_x / _y */
  int32_t obs_dim;                       /* rows of the observation (PGTT_OBS or the baseline's) */
  int32_t scan_row0;                     /* first scan row of the observation; scan_row0 + PGTT_NSCAN <= obs_dim */
} PgttElevationConfig;

/* device pointers, all caller-owned, sized for N = num_envs given to pgtt_elevation_create */
typedef struct PgttElevationBuffers {
  const float* state;                    /* [PGTT_NSTATE][N] (PgttBuffers.state), required */
  const float* depth;                    /* [N][H][W] (PgttDepthBuffers.depth), required */
  const float* obs;                      /* [N][obs_dim] (PgttBuffers.obs_state); required with obs_out, else may be NULL */
  const float* done;                     /* [N] 0 / 1 (PgttBuffers.done) or NULL: use_done then clears nothing */
  float* map;                            /* [N][G][G], required; NaN = unknown */
  int32_t* origin;                       /* [N][2], required */
  float* est;                            /* [N][PGTT_NSCAN], required */
  uint8_t* known;                        /* [N][PGTT_NSCAN], required */
  float* obs_out;                        /* [N][obs_dim] or NULL */
} PgttElevationBuffers;

typedef struct pgtt_elevation_map* pgtt_elevation_handle;

/* the config's checks alone: host only, needs no GPU.  PGTT_E_ARG for a config outside the ranges above. */
int pgtt_elevation_check(const PgttElevationConfig* cfg);
int pgtt_elevation_create(const PgttElevationConfig* cfg, int device, int num_envs, pgtt_elevation_handle* out);
int pgtt_elevation_destroy(pgtt_elevation_handle h);
/* PGTT_E_ARG when a required pointer is NULL.  A pgtt_elevation() captured in a HIP graph keeps the pointers bound at capture. */
int pgtt_elevation_bind(pgtt_elevation_handle h, const PgttElevationBuffers* bufs);
/* one tick for all N envs: one launch, one workgroup of 256 lanes per env.  clear_mask: device uint8 [N] or NULL.
 * PGTT_E_STATE before pgtt_elevation_bind. */
int pgtt_elevation(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream);
/* As pgtt_elevation_bind, but bufs->depth may be NULL, and `points` (device [N][P][3], world frame) is required with P >= 1 (PGTT_E_ARG).
 * pgtt_elevation_bind afterwards unbinds the points. */
int pgtt_elevation_bind_points(pgtt_elevation_handle h, const PgttElevationBuffers* bufs, const float* points, int P);
/* one tick for all N envs from the bound points: one launch, as pgtt_elevation().  PGTT_E_STATE before pgtt_elevation_bind_points; pgtt_elevation()
 * on a handle bound with depth == NULL is PGTT_E_STATE too. */
int pgtt_elevation_points(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream);

/* device pointers of the hole filling's outputs, caller-owned, sized for N */
typedef struct PgttElevationFill {
  float* est;                            /* [N][PGTT_NSCAN], required */
  uint8_t* dist;                         /* [N][PGTT_NSCAN], required: 0 measured, 1..passes the pass that filled it, 255 unknown */
  float* obs_out;                        /* [N][obs_dim] or NULL */
  float* map_out;                        /* [N][G][G] or NULL */
  uint8_t* dist_out;                     /* [N][G][G] or NULL */
} PgttElevationFill;

/* PGTT_E_ARG for a NULL struct, a NULL required pointer or passes outside 1 .. PGTT_ELEVATION_MAX_GRID - 1.  May be called before or after the
 * buffers are bound; the binding persists across later pgtt_elevation_bind / pgtt_elevation_bind_points. */
int pgtt_elevation_bind_fill(pgtt_elevation_handle h, const PgttElevationFill* out, int passes);
/* the hole filling for all N envs: one launch on `stream`, one workgroup of 256 lanes per env, no allocation and no synchronisation, so it can be
 * captured.  PGTT_E_STATE before the buffers are bound (either kind of bind) or before pgtt_elevation_bind_fill; PGTT_E_ARG when the fill's obs_out
 * is bound and the buffers' obs is NULL. */
int pgtt_elevation_fill(pgtt_elevation_handle h, void* stream);
/* counter: the SENSOR's device counter (PgttDepthBuffers.counter or PgttLidarBuffers.counter), every: that sensor's period, >= 1.
 * PGTT_E_ARG for a NULL counter or every < 1.  May be called before or after the buffers are bound and persists across later binds, like
 * pgtt_elevation_bind_fill. */
int pgtt_elevation_bind_rate(pgtt_elevation_handle h, const int64_t* counter, int every);
/* Called BEHIND the sensor's call of the same step, with the `force` that call was given.  PGTT_E_STATE before a bind of the buffers or before
 * pgtt_elevation_bind_rate.  The image or the points are used, by which bind was made last (as pgtt_elevation / pgtt_elevation_points). */
int pgtt_elevation_follow(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, int force, void* stream);

#define PGTT_ELEVATION_MAX_BAND 0.5f             /* band <= 0.5 m: q < 2^18, and 65536 pixels of one cell sum below 2^34 */
#define PGTT_ELEVATION_BAND_SCALE 262144.0f      /* 2^18: the band offsets are summed as integers in units of 2^-18 m */
#define PGTT_ELEVATION_VAR_MAX_GRID 64           /* 12 * 64 * 64 = 49152 bytes of LDS */

/* the variance layer: its two caller-owned device buffers, sized for N, and its settings (all finite) */
typedef struct PgttElevationVar {
  float* var;                            /* [N][G][G], required; NaN where map is NaN */
  float* est_var;                        /* [N][PGTT_NSCAN], required */
  float sigma0;                          /* range-independent standard deviation, metres, >= 0 */
  float sigma_rel;                       /* standard deviation per metre of distance, >= 0, and sigma0 + sigma_rel > 0 */
  float process;                         /* variance added to every known cell per tick, m^2, >= 0 */
  float gate;                            /* Mahalanobis gate, > 0 */
  float band;                            /* thickness of the upper-surface band, metres, 0 <= band <= PGTT_ELEVATION_MAX_BAND */
  int32_t max_count;                     /* cap on the number of pixels of one cell that count as independent, >= 1 */
  float var_max;                         /* prior variance and clamp, m^2, > 0 */
} PgttElevationVar;

/* the settings' ranges alone (the pointers are not looked at): host only, needs no GPU.  PGTT_E_ARG for NULL or a value outside its range. */
int pgtt_elevation_check_var(const PgttElevationVar* v);
/* PGTT_E_ARG for a NULL struct, a NULL var or est_var, a value outside its range, or a handle whose grid is above PGTT_ELEVATION_VAR_MAX_GRID.
 * May be called before or after the buffers are bound and persists across later binds, like pgtt_elevation_bind_fill. */
int pgtt_elevation_bind_var(pgtt_elevation_handle h, const PgttElevationVar* v);
/* one variance tick for all N envs from the image: ONE launch on `stream`, no allocation, no synchronisation, no read-back, capturable.
 * PGTT_E_STATE before the buffers are bound, on a handle bound without a depth image, or before pgtt_elevation_bind_var. */
int pgtt_elevation_var(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream);
/* the same from the bound points (the source is whichever bind was made last, as for pgtt_elevation_points): PGTT_E_STATE before
 * pgtt_elevation_bind_points or before pgtt_elevation_bind_var. */
int pgtt_elevation_var_points(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream);

#define PGTT_RS_ODOMETRY 34                      /* Philox stream id of the odometry draws (pgtt.h uses ids below 32, the depth camera 32, the LiDAR 33) */
#define PGTT_ELEVATION_ODO_WORDS 12              /* floats of persistent odometry state per env */

/* the odometry call's device buffers, caller-owned and sized for N, and its settings (all finite) */
typedef struct PgttElevationOdometry {
  const float* state;                    /* the TRUE state: [PGTT_NSTATE][N] (PgttBuffers.state) or any [>= 7][N]; rows 0..6 are read; required */
  const float* done;                     /* [N] 0 / 1 or NULL: use_done then clears nothing */
  const float* points;                   /* [N][P][3] world points registered at the true pose, or NULL */
  float* points_est;                     /* [N][P][3], required with points and NULL without */
  int32_t P;                             /* >= 1 with points */
  float* pose_est;                       /* [7][N], required: a legal `state` of every entry of this library */
  float* odo;                            /* [N][PGTT_ELEVATION_ODO_WORDS], required; the first call clears it (clear_all) */
  int64_t* counter;                      /* [1], required: the epoch of the draws, advanced by one per call */
  uint64_t seed;                         /* key of the Philox draws */
  int64_t env_id_offset;                 /* global id of env 0 */
  float dt;                              /* seconds between two calls (the control step), > 0 */
  float sigma_xy, sigma_z;               /* position random walk per sqrt(metre walked), >= 0 */
  float sigma_yaw;                       /* yaw random walk, rad / sqrt(s), >= 0 */
  float yaw_bias;                        /* bound of the episode's gyro bias, rad / s, >= 0 */
  float scale;                           /* bound of the episode's odometry scale error, 0 <= scale < 1 */
} PgttElevationOdometry;

/* the settings' ranges alone (the pointers and P are not looked at): host only, needs no GPU.  PGTT_E_ARG for NULL or a value outside its range. */
int pgtt_elevation_check_odometry(const PgttElevationOdometry* o);
/* PGTT_E_ARG for a NULL struct, a NULL state, pose_est, odo or counter, points without points_est or the other way round, points with P < 1, or
 * a setting outside its range.  May be called before or after the buffers are bound and persists across later binds, like pgtt_elevation_bind_fill. */
int pgtt_elevation_bind_odometry(pgtt_elevation_handle h, const PgttElevationOdometry* o);
/* one odometry update for all N envs, called BEFORE the tick that reads pose_est: two launches on `stream` (the update; the counter), no allocation,
 * no synchronisation, no read-back, capturable.  Without points one lane per env, with points one workgroup of 256 lanes per env.
 * PGTT_E_STATE before pgtt_elevation_bind_odometry. */
int pgtt_elevation_odometry(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream);
int pgtt_elevation_sizeof_odometry(void);
int pgtt_elevation_sizeof_var(void);
int pgtt_elevation_sizeof_fill(void);
int pgtt_elevation_sizeof_config(void);
int pgtt_elevation_sizeof_buffers(void);

/* Visibility clean-up: its settings (all finite) and its two caller-owned device outputs, sized for N */
typedef struct PgttElevationVisibility {
  float margin;                          /* metres, > 0: a cell is contradicted when h (see sigmas) > bound + margin */
  float end_guard;                       /* metres, >= 0: samples closer than this (horizontally) to the ray's end point are not made */
  int32_t stride;                        /* >= 1: image pixels with i % stride == 0 and j % stride == 0 cast a ray; points with k % stride == 0 */
  float sigmas;                          /* >= 0, read only with a variance layer bound: h is replaced by h - sigmas * sqrtf(v) in the test */
  float sensor_pos[3];                   /* points source only: the sensor's position in the BASE frame (the image source uses cfg.mount_pos) */
  int32_t* cleared;                      /* [N], required: cells set to NaN by this call */
  float* bound_out;                      /* [N][G][G] or NULL: the bound layer in the slot layout of `map`, NaN = no sample fell into the cell */
} PgttElevationVisibility;

/* the settings' ranges alone (the pointers are not looked at): host only, needs no GPU.  PGTT_E_ARG for NULL or a value outside its range. */
int pgtt_elevation_check_visibility(const PgttElevationVisibility* v);
/* PGTT_E_ARG for a NULL struct, a NULL cleared or a setting outside its range.  May be called before or after the buffers are bound and persists
 * across later binds, like pgtt_elevation_bind_fill. */
int pgtt_elevation_bind_visibility(pgtt_elevation_handle h, const PgttElevationVisibility* v);
/* the clean-up for all N envs, called BEFORE the tick of the same step with that tick's clear arguments: ONE launch on `stream`, no allocation, no
 * synchronisation, no read-back, capturable.  PGTT_E_STATE before the buffers are bound (either kind of bind) or before
 * pgtt_elevation_bind_visibility. */
int pgtt_elevation_visibility(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream);
int pgtt_elevation_sizeof_visibility(void);

#define PGTT_RS_LATENCY 35                       /* Philox stream id of the latency draws (pgtt.h uses ids below 32, the depth camera 32, the LiDAR 33, the odometry 34) */
#define PGTT_ELEVATION_MAX_LATENCY 8             /* ticks */

/* Sensor latency: the ring, the per-env bookkeeping (device buffers, caller-owned and sized for N) and the range of the draws */
typedef struct PgttElevationLatency {
  float* ring_data;                      /* image source: [D][N][H][W]; points source: [D][N][P][3]; required */
  float* ring_pose;                      /* [D][7][N]: rows 0..6 of the bound `state` at capture, raw; required */
  int32_t* lat;                          /* [N]: the env's latency of this episode, in calls; required */
  int32_t* age;                          /* [N]: frames pushed since the env was last cleared, saturating at D; required */
  uint8_t* fused;                        /* [N] out: 1 when this call fused a frame for the env, else 0; required */
  int64_t* counter;                      /* [1]: calls so far; advanced by one per call; required */
  int32_t D;                             /* ring slots, lat_hi + 1 <= D <= PGTT_ELEVATION_MAX_LATENCY + 1 */
  int32_t lat_lo, lat_hi;                /* 0 <= lat_lo <= lat_hi <= PGTT_ELEVATION_MAX_LATENCY */
  uint64_t seed;                         /* key of the Philox draws */
  int64_t env_id_offset;                 /* global id of env 0 */
} PgttElevationLatency;

/* the ranges alone (the pointers are not looked at): host only, needs no GPU.  PGTT_E_ARG for NULL or a value outside its range. */
int pgtt_elevation_check_latency(const PgttElevationLatency* l);
/* PGTT_E_ARG for a NULL struct, a NULL pointer or a value outside its range.  May be called before or after the buffers are bound and persists
 * across later binds, like pgtt_elevation_bind_fill.  The ring's frames are those of the source bound when pgtt_elevation_delayed is called. */
int pgtt_elevation_bind_latency(pgtt_elevation_handle h, const PgttElevationLatency* l);
/* the tick of a handle with a latency bound, from the image or the points, by which bind was made last: at most three launches on `stream` (the
 * push; the stamped tick; the counter), no allocation, no synchronisation, no read-back, capturable.  PGTT_E_STATE before the buffers are bound
 * (either kind of bind) or before pgtt_elevation_bind_latency. */
int pgtt_elevation_delayed(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream);
int pgtt_elevation_sizeof_latency(void);
/* "src=<SHA-256 of pgtt_elevation.hip and the files it includes>;flavor=product" */
const char* pgtt_elevation_build_info(void);
const char* pgtt_elevation_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PGTT_ELEVATION_H_ */
