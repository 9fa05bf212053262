/*
 * pbr_hip_diag.h — diagnostic entry points of libpbrhip.so.
 *
 * Not part of the drop-in boundary (the reference has nothing comparable): they expose single
 * stages of the device path — the math layer, closest-hit traversal, BRDF evaluation, new-ray
 * sampling, the cubic solver and the patch intersection of Phong tessellation, the camera ray, the
 * intersection primitives of the walk (triangle, box, sphere) and the surface step of a bounce — so the parity tests
 * can compare each stage with the oracle's hook of the same shape (oracle/pt_oracle.h: orc_math,
 * orc_trace_rays, orc_brdf_eval, orc_new_ray, orc_solve_cubic, orc_phong_face, orc_camera_ray, orc_intersect,
 * orc_surface_step) instead of only whole
 * images, and with float64 references.  Host pointers in, host pointers out; synchronous.
 *
 * pbr_diag_math, pbr_diag_brdf, pbr_diag_new_ray, pbr_diag_solve_cubic, pbr_diag_phong_face, pbr_diag_camera_ray,
 * pbr_diag_intersect and pbr_diag_surface_step compute in the arithmetic
 * of the context's last successful pbr_configure: the native one (v_sin / v_rcp / v_log / ... , csrc/pt_math.hpp) when it
 * set arith = PBR_ARITH_NATIVE, the exact one — the oracle's definitions, bit for bit — with no configuration or arith =
 * exact.  A library built without the native diagnostics answers PBR_ESTATE in the native case.  pbr_diag_trace is always
 * exact.
 */
#ifndef PBR_HIP_DIAG_H
#define PBR_HIP_DIAG_H

#include "pbr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* op: 0 sin, 1 cos, 2 tan, 3 acos, 4 atan, 5 pow( x, y ), 6 fract( sin( x ) * 43758.5453123 ), 7 cbrt (binary64 in both
 * arithmetics) */
int pbr_diag_math( pbr_ctx* ctx, int op, const float* x, const float* y, int n, float* out );

/* Closest-hit traversal (pt_bvh.cl:82-123) of n rays {origin, dir} against the uploaded scene, in the walk of the
 * configured traversal, always in the exact arithmetic.
 * out_t[n], out_face[n], out_normal[3n] (0 on a miss), out_counts[2n] = {node visits, face tests}.
 * Follows the configuration as orc_trace_rays does: with phong_tessellation > 0 configured and a scene whose vertex
 * normals were usable it runs the Phong-tessellation build of the walk (curved faces as patches) and out_normal is the
 * hit's own normal — the patch normal of a curved face; otherwise flat triangles and the face's geometric normal. */
int pbr_diag_trace( pbr_ctx* ctx, const float* rays, int n, float* out_t, int32_t* out_face, float* out_normal, uint32_t* out_counts );

/* BRDF evaluation with material 0 of the uploaded scene.  in: n x 16 {out_dir[3], in_dir[3],
 * normal[3], pad[7]}; out: n x 4 — BRDF 0 {brdf, u, pdf, 0}, BRDF 1 {spec, diff, dotHK1, pdf}. */
int pbr_diag_brdf( pbr_ctx* ctx, const float* in, int n, float* out );

/* getNewRay (pt_brdf.cl:344-378) with material 0.  in: n x 12 {origin[3], dir[3], normal[3], t,
 * seed, pad}; out: n x 8 {origin[3], dir[3], seed after, addDepth}. */
int pbr_diag_new_ray( pbr_ctx* ctx, const float* in, int n, float* out );

/* solveCubic (pt_utils.cl:108-199) alone, no scene needed.  in: n x 4 {a0, a1, a2, a3} of a0 x^3 + a1 x^2 + a2 x + a3;
 * out: n x 4 {count, x0, x1, x2}, the slots beyond count written as 0 (orc_solve_cubic). */
int pbr_diag_solve_cubic( pbr_ctx* ctx, const float* in, int n, float* out );

/* phongTessTriAndRayIntersect (pt_phongtess.cl:56-212) alone, no scene needed: called directly, not through the face test
 * that sends a face with three equal normals to the flat intersection, so near-equal and equal normals reach it.
 * in: n x 32 {P1[3], P2[3], P3[3], N1[3], N2[3], N3[3], origin[3], dir[3], rayT, tNear, tFar, alpha, pad[4]};
 * out: n x 4 {t (INFINITY: no hit), normal[3] (0 on a miss)} (orc_phong_face).
 * tNear / tFar are the slab interval of the leaf's box as the walk hands them over.  A hit is accepted only for
 * |tNear| <= t <= min( rayT, tFar ) (pt_phongtess.cl:202): for an origin INSIDE the box tNear is negative, and hits nearer
 * than |tNear| are dropped.  That is the reference's behaviour, kept as it is — which is why the interval is an input here. */
int pbr_diag_phong_face( pbr_ctx* ctx, const float* in, int n, float* out );

/* initRay with anti-aliasing and the depth-of-field lens (pathtracing.cl:25-48, pt_utils.cl:327-373) for n pixels of the
 * camera `cam` at pixel dimension pxDim.  Width, height and anti-aliasing are the configuration's (PBR_ESTATE without one);
 * the kernel is handed the camera exactly as a render call's kernels are.
 * in: n x 8 {px, py, seed, tFocus, tObject, pad[3]} (px, py whole numbers; tFocus / tObject as getPreviousFocus gives them:
 * -1 = depth of field off); out: n x 8 {origin[3], dir[3], seed after, 0} — the seed after tells the draws taken: 2, or 4
 * with the lens (orc_camera_ray). */
int pbr_diag_camera_ray( pbr_ctx* ctx, float pxDim, const pbr_camera* cam, const float* in, int n, float* out );

/* The primitives of the walk alone, no scene needed.  in: n x 24, out: n x 4 (orc_intersect).
 * op 0, flatTriAndRayIntersect (pt_intersect.cl:92-129) on the face record the upload forms (B - A, C - A in binary32):
 *   in {A[3], B[3], C[3], origin[3], dir[3], rayT, tNear, pad[7]}; out {t (INFINITY: no hit), 0, 0, 0}
 * op 1, intersectBox (pt_intersect.cl:11-25) with the inverse direction of the walk, and the hit conditions of the
 *   closest-hit walk (pt_bvh.cl:107-110) and of the shadow walk (:151-154, no `rayT > tNear` cull):
 *   in {min[3], max[3], origin[3], dir[3], rayT, pad[11]}; out {closest-hit verdict, any-hit verdict, tNear, tFar}
 * op 2, intersectSphere (pt_intersect.cl:37-77; d2 is compared with r, not r * r, as the reference does):
 *   in {pos[3], r, origin[3], dir[3], pad[14]}; out {hit, tNear (0 on a miss), 0, 0} */
int pbr_diag_intersect( pbr_ctx* ctx, int op, const float* in, int n, float* out );

/* The surface step of one bounce with material 0 and the scene's BRDF: getNewRay's direction from the unflipped normal, the
 * normal flip (pathtracing.cl:298-300), then updateColor (pathtracing.cl:89-178) — the shadow-ray contribution when `lit`,
 * and the throughput factor.
 * in: n x 24 {origin[3], dir[3], normal[3] (unflipped), t, seed, color[3], lit (0 / 1), lightDir[3], lightRgb[3], pad[3]};
 * out: n x 12 {newDir[3], seed after, addDepth, color after[3], finalColor after starting from 0 [3], secondaryPaths
 * increment} (orc_surface_step). */
int pbr_diag_surface_step( pbr_ctx* ctx, const float* in, int n, float* out );

/* The a-trous filters over planes the caller supplies — kind 0: pbr_denoise's passes (ptd::atrousPass), kind 1: those of
 * pbr_denoise_guided and pbr_denoise_temporal (ptd::atrousGuidedPass) — through the pass drivers the public calls use: same
 * grid and block, same by-value arguments per pass, same ping-pong, same last pass (the guided filter's `original` is `image`).
 * Needs a live context for its device and stream only: no scene, no pbr_configure; it touches none of the context's images,
 * moments, history, counters or kernel time.
 *   width, height  >= 1, width * height <= 1 Mi; NOT bound to multiples of 8
 *   params         pbr_denoise_params (kind 0) / pbr_denoise_guided_params (kind 1): passes 1 .. 8, standard deviations
 *                  finite and >= 0, as the public calls check them
 *   image          width x height x 4: colour, .w = the first-hit distance that passes through
 *   variance       width x height, V_0 (kind 1; ignored and may be NULL for kind 0)
 *   features       3 x width x height x 4: position, normal, albedo as pbr_denoise returns them
 *   rgba_out       width x height x 4;  variance_out: width x height, kind 1, may be NULL
 * PBR_EINVAL for anything else; a refused or failed call writes nothing. */
int pbr_diag_filter( pbr_ctx* ctx, int kind, int width, int height, float pxDim, const void* params, const float* image, const float* variance,
                     const float* features, float* rgba_out, float* variance_out );

/* Steps 0 to 4 of pbr_denoise_temporal (pbr_hip.h: the motion step, the candidate, the taps, the history value, the blend) over
 * planes the caller supplies, through the driver the public call uses: same grid and block, the same by-value arguments built
 * from the two cameras, ptd::temporalMotion in front of ptd::temporalIntegrate< true > on the motion path, else
 * ptd::temporalIntegrate< false > alone.  No filter pass follows.  Needs a live context for its device and stream only: no
 * scene, no pbr_configure; it touches none of the context's images, moments, history, motion policy, counters or kernel time.
 *   width, height  >= 1, width * height <= 1 Mi; NOT bound to multiples of 8
 *   pxDim, cam     of this call;  temporal: checked as pbr_denoise_temporal checks it
 *   image          width x height x 4, variance: width x height — merged into {r, g, b, var} as the public call's working plane is
 *   features       3 x width x height x 4: position, normal, albedo as pbr_denoise returns them
 *   previous state prev_integrated (w x h x 4), prev_features (3 x w x h x 4), prev_lengths (w x h), prev_cam, prev_pxDim: all of
 *                  the four pointers, or none (NULL) — none is the first call after a reset: every pixel copies, L = 1
 *   motion inputs  face (w x h, -1 = miss), facesV (num_faces x 4: {a, b, c, material}), vertices and hist_vertices
 *                  (num_vertices x 4: V and H): all four, or none.  All four: the motion path
 *   integrated     w x h x 4;  history: w x h x 4 {fx, fy, L, valid};  lengths: w x h
 *   motion         w x h x 4 {Pprev, code}, reference: w x h x 4 {nref, len} — step 0's two planes; written on the motion path
 *                  only (required there, ignored otherwise)
 * PBR_EINVAL for a null or size error, a previous state or motion inputs given in part, motion inputs without a previous
 * state, more than 16 Mi faces or vertices, a face outside [-1, num_faces), a facesV corner >= num_vertices — the two keep the
 * kernels' gathers in bounds — and a prev_lengths entry outside 1 .. 1024.  The last keeps Hl + 1 inside the definition: the
 * kernel forms it in 32-bit unsigned arithmetic, the definition (and the tests' restatement, in 64-bit integers) in the
 * integers; the two agree for every length a call of the library can have left — 1 .. max_history <= 1024 — and need not
 * beyond 2^32 - 2.  A refused or failed call writes nothing. */
int pbr_diag_temporal( pbr_ctx* ctx, int width, int height, float pxDim, const pbr_camera* cam, const pbr_temporal_params* temporal,
                       const float* image, const float* variance, const float* features,
                       const float* prev_integrated, const float* prev_features, const uint32_t* prev_lengths, const pbr_camera* prev_cam, float prev_pxDim,
                       const int32_t* face, const uint32_t* facesV, uint32_t num_faces, const float* vertices, const float* hist_vertices, uint32_t num_vertices,
                       float* integrated, float* history, uint32_t* lengths, float* motion, float* reference );

/* Traversal-only throughput probe: streams n rays {ox,oy,oz,-, dx,dy,dz,-} through a persistent
 * closest-hit kernel `repeats` times with `lds_slots` hot nodes staged in LDS; best kernel time in
 * *ms_out, hits {t, face bits} in out2. */
int pbr_diag_trace_stream( pbr_ctx* ctx, int lds_slots, const float* rays8, uint32_t n, int repeats, float* out2, double* ms_out );

/* One chosen ray per thread through the walk the lock-step render kernels run (csrc/pt_walk_diag.hpp): traverse() of the
 * context's build flavour — the configured traversal AND arithmetic, unlike pbr_diag_trace — behind the staged prefix, the
 * closest-hit walk (anyhit = 0) or the shadow walk of the shade step (anyhit = 1), which no other entry reaches.  With
 * lds_slots > 0 a product build walks through the hand-scheduled node phases (nodePhaseAsm / nodePhaseAsmCompact), a
 * PBR_GUARD build through the C++ loop over LDS; with 0 both walk the C++ loop on the stream in memory.
 *   rays8       n x { origin.xyz, t0 }{ dir.xyz, - } — pbr_diag_trace_stream's layout.  t0 is what hit.t starts from: the
 *               distance of the light for the any-hit walk; +inf for the closest-hit walk, or a finite bound (a box whose
 *               tNear is not below it is culled)
 *   lds_slots   the 32-byte slots of the node stream a block stages, clamped as pbr_diag_trace_stream clamps them: to the
 *               ranked prefix, to a block's share of LDS, to whole records of the compact layout (traversal 3: even)
 *   out_t, out_face, out_normal, out_counts   as pbr_diag_trace.  The any-hit walk reports the ray as traverse() leaves it:
 *               t < t0 blocked, t >= t0 lit (t may exceed t0: an orb light in front of t0 sets it to inf, faces behind the
 *               light are then recorded and do not stop the walk); its normal is 0 and its node visits are 0 — the shadow
 *               walk does not count them, as in the reference.  A closest-hit ray that found nothing below a finite t0
 *               returns t = t0, face 0, normal 0.
 * One launch, thread i walks ray i in blocks of 1024: rays 64 w .. 64 w + 63 share wave w and its node phases, so the caller
 * decides who parks with whom; the last wave runs with n % 64 lanes.  Lights, Phong tessellation: as pbr_diag_trace.  The park
 * share is a render's (knob "park_eighths").  PBR_EDEVICE if the staged prefix was not at LDS address 0. */
int pbr_diag_trace_walk( pbr_ctx* ctx, int anyhit, int lds_slots, const float* rays8, uint32_t n,
                         float* out_t, int32_t* out_face, float* out_normal, uint32_t* out_counts );

/* What pbr_diag_trace_walk makes of a request of lds_slots under the uploaded scene and the configured traversal: *slots = the
 * 32-byte slots a block would stage, *hot_slots (may be NULL) = the ranked prefix of the node stream that bounds them.  No launch. */
int pbr_diag_trace_walk_slots( pbr_ctx* ctx, int lds_slots, uint32_t* slots, uint32_t* hot_slots );

/* Memory-counter calibration: reads `reads` elements of a zero-filled table of table_bytes in a
 * known pattern (mode 0 coalesced 16 B / lane stream, 1 random 16-B elements, 2 random 32-B
 * records) so that rocprofv3's FETCH_SIZE / TCC_EA0_RDREQ_* can be interpreted. */
int pbr_diag_calibrate( pbr_ctx* ctx, int mode, uint64_t table_bytes, uint64_t reads, double* ms_out );

/* Which schedule rendered (the largest chunk of) the last render: "refill-lean", "refill-wide", "phased-lean",
 * "phased-wide", "phased-mid", "refill-mid", "phased-dual" ("refill-lean-phong" with Phong tessellation); *tuned = index of the schedule the auto-tuner
 * settled on for this scene + configuration, or -1 while it is still measuring (pbr_hip.hip, launch()). */
int pbr_diag_last_plan( pbr_ctx* ctx, char* name, size_t capacity, int* tuned );

/* pbr_build_bvh: the search radius the clustering builder used in this context's last build — 32 when the context was
 * configured for the reference's walk (or not configured yet) at the time of the call, 3 when it was configured for a
 * ray-ordered walk, or the "ploc_radius" knob (0: no build yet).  The protocol: pbr_configure (with the traversal the tree
 * will be walked in) BEFORE pbr_build_bvh; this call shows which one a build got. */
int pbr_diag_bvh_build_info( pbr_ctx* ctx, int* radius );

/* Device memory of the uploaded scene's arrays, bytes: [0] the node stream in the reference's order, [1] the streams of
 * the ray-ordered walk (0 unless such a mode is configured: six or eight times [0], compact records twice [0]), [2] the face records.
 * Not in these figures: what the upload keeps for pbr_update_vertices — 16 bytes per face and per vertex, 10 per node, 4 per
 * thread slot of the refit's workgroups; pbr_diag_refit_info below reports it. */
int pbr_diag_scene_bytes( pbr_ctx* ctx, uint64_t out[3] );

/* What pbr_upload_scene keeps for pbr_update_vertices (csrc/pt_refit_host.hpp), beyond pbr_diag_scene_bytes' three figures:
 * out[0] 1 if the tree can be refitted (properly nested; else `why` holds the reason), [1] the cap S of a subtree's nodes,
 * [2] the workgroups of the subtree kernel, [3] the maximal subtrees of at most S nodes they share, [4] the nodes above the
 * cut and [5] their levels (one more launch), [6] the device bytes kept for updates — 16 per face (its vertex indices), 16 per
 * vertex, 10 per node (a word, a height, its record) and 4 per thread slot of [2] x S, nothing for a tree that cannot be
 * refitted —, [7] the updates since the upload.  *upload_ms: the host's time inside the copy of the last update's vertices to
 * the device (pbr_last_kernel_ms excludes it).  upload_ms and why may be NULL. */
int pbr_diag_refit_info( pbr_ctx* ctx, uint64_t out[8], double* upload_ms, char* why, size_t capacity );

/* pbr_update_geometry (pbr_hip.h): out[0] 1 if the scene has Phong patch records (usable vertex normals at the upload), [1] the
 * device bytes of the patch refit's tables as they are held now — 16 per face, 16 per normal, 24 per face; 0 until the first
 * pbr_update_geometry after an upload —, [2] the successful pbr_update_geometry calls since the upload, [3] 1 if the most recent
 * successful update was one of them (pbr_configure's state rule).  *alpha (may be NULL): the phong_tessellation that update
 * built its boxes with.  pbr_diag_refit_info's figures do not include any of this; its upload_ms covers the copy of the normals
 * too when the last update was a pbr_update_geometry that brought some.  PBR_EINVAL for a null context or null out,
 * PBR_ESTATE without a scene. */
int pbr_diag_patch_refit_info( pbr_ctx* ctx, uint64_t out[4], float* alpha );

/* pbr_set_parts / pbr_update_transforms (pbr_hip.h): out[0] the parts (0 if none are set), [1] the device bytes held for them —
 * 36 per vertex (rest position, staging position, part index), 20 per normal if normal parts are set, 96 per part, 4 of a flag
 * word —, [2] the successful pbr_update_transforms calls since pbr_set_parts, [3] 1 if the most recent successful update of any
 * kind was one of them.  *ms (may be NULL): the device time of the transform kernels alone in that update; pbr_last_kernel_ms
 * covers the whole update.  pbr_set_parts also makes pbr_update_geometry's tables when the scene has patches:
 * pbr_diag_patch_refit_info's bytes are then no longer 0 before the first update.  PBR_EINVAL for a null context or null out. */
int pbr_diag_transform_info( pbr_ctx* ctx, uint64_t out[4], double* ms );

/* pbr_set_skin / pbr_update_skin (pbr_hip.h): out[0] the bones (0 if no skin is set), [1] the device bytes held for the skin —
 * 64 per vertex (rest position, staging position, 32-byte influence record), 48 per normal if normal influences are set, 48
 * per bone, 4 of a flag word: 64 V + 48 N + 48 bones + 4 —, [2] the successful pbr_update_skin calls since pbr_set_skin,
 * [3] 1 if the most recent successful update of any kind was one of them.  *ms (may be NULL): the device time of the skin
 * kernels alone in that update; pbr_last_kernel_ms covers the whole update.  PBR_EINVAL for a null context or null out. */
int pbr_diag_skin_info( pbr_ctx* ctx, uint64_t out[4], double* ms );

/* pbr_set_morph / pbr_update_morph / pbr_update_pose (pbr_hip.h): out[0] the targets (0 if no morph is set), [1] the vertex
 * entries Ev, [2] the normal entries En, [3] the device bytes held for the morph — 16 V + 16 V + 4 ( V + 1 ) + 16 Ev (rest
 * position, staging position, runs, entries), + 16 N + 4 ( N + 1 ) + 16 En with normal targets, + 4 T + 4 (weight table, flag
 * word) —, [4] the successful pbr_update_morph and pbr_update_pose calls since pbr_set_morph, [5] the most recent successful
 * update of any kind: 0 none of the two, 1 a pbr_update_morph, 2 a pbr_update_pose.  *ms (may be NULL): the device time of the
 * morph / pose kernels alone in that update; pbr_last_kernel_ms covers the whole update.  PBR_EINVAL for a null context or null
 * out. */
int pbr_diag_morph_info( pbr_ctx* ctx, uint64_t out[6], double* ms );

/* pbr_update_skin_dq / pbr_update_pose_dq (pbr_hip.h): out[0] the successful calls of the two since pbr_set_skin (a new
 * pbr_set_skin, dropping the skin and pbr_upload_scene start it again at 0), [1] the most recent successful update of any kind:
 * 0 none of the two, 1 a pbr_update_skin_dq, 2 a pbr_update_pose_dq.  *ms (may be NULL): the device time of the dq kernels alone
 * in the last of them; pbr_last_kernel_ms covers the whole update.  The dual quaternions lie in the 48 bytes per bone that
 * pbr_set_skin allocated, so pbr_diag_skin_info's bytes are the same with and without them.  To pbr_diag_skin_info and
 * pbr_diag_morph_info a dq update is another kind: their counts and times do not move, their last_update is 0 afterwards.
 * PBR_EINVAL for a null context or null out. */
int pbr_diag_skin_dq_info( pbr_ctx* ctx, uint64_t out[2], double* ms );

/* The Phong patch records as they are on the device now: six quads per face, the corners, then the vertex normals, .w = 0.
 * *count = the quads; out = NULL returns the count only, else capacity >= *count quads.  PBR_ESTATE without a scene or for a
 * scene without usable vertex normals, PBR_EINVAL for a null context, null count or too little room. */
int pbr_diag_read_patches( pbr_ctx* ctx, pbr_float4* out, uint32_t capacity, uint32_t* count );

/* The configured ray-ordered layout's device buffer as it is now, header included (pbr_refit_ordered_walk's contract is stated
 * on these bytes): *bytes = its size, first[8] = the context's eight first references, *hot_slots = the 32-byte slots at the head
 * of the records that are ranked for LDS staging (first and hot_slots may be NULL).  out = NULL returns these only, else
 * capacity >= *bytes.  PBR_ESTATE when no ordered stream is built, PBR_EINVAL for a null context, null bytes or too little room. */
int pbr_diag_read_walk( pbr_ctx* ctx, void* out, uint64_t capacity, uint64_t* bytes, int first[8], uint32_t* hot_slots );

/* The re-link of pbr_update_vertices (pbr_refit_ordered_walk; csrc/pt_relink_host.hpp): out[0] the device bytes of its tables as
 * they are held now (0: none), [1] the top-down levels of the tree they were built for, [2] the kernel launches of the last
 * update's re-link, [3] 1 if the last pbr_update_vertices re-linked, else 0.  *ms (may be NULL): the device time of those
 * launches alone; pbr_last_kernel_ms includes it. */
int pbr_diag_relink_info( pbr_ctx* ctx, uint64_t out[4], double* ms );

/* The kernel behind pbr_diag_last_plan's schedule, as a profiler prints its symbol (without "void " and the argument
 * list): "ptk_f0::pathTracingDual<1, false, false>" — namespace ptk_f<flavour> (bit 0: ray-ordered walk, bit 1: native
 * arithmetic; csrc/pt_flavour.hpp), template arguments BRDF, SHADOW_RAYS, LIGHTS[, waves per SIMD[, PHONGTESS]]. */
int pbr_diag_last_kernel( pbr_ctx* ctx, char* name, size_t capacity );

/* What the schedule tuner measured for the plan in use: a launch of n frames costs fixed_ms + n * per_frame_ms (least
 * squares over its refinement launches of two lengths; fixed_ms = the ramp-up of a launch and the drain of its longest
 * paths).  PBR_ESTATE when there is no such fit (plan pinned before the tuner ran, single-length launches only). */
int pbr_diag_launch_fit( pbr_ctx* ctx, double* fixed_ms, double* per_frame_ms );

/* Experiment and test knobs, per context; value -1 = the built-in default.  The library reads NO environment variable:
 * lab scripts and tests that need a knob set it here (the Python harness maps PBR_* variables onto this call).
 *   "lds_slots"     cap of the node records a block stages in LDS (0 = none)
 *   "blocks_per_cu" run below the resident maximum
 *   "ph_park" / "ph_shade"  lane state machine thresholds (phased-dual: ph_park counts walks of up to 128 per wave); "park_eighths": the lock-step walk's park share
 *   "drain_mode"    bit 0 / 1: scale ph_park / ph_shade with the lanes still at work once the queue is empty
 *   "refill_batch"  lock-step kernels: lanes of a wave that wait with a finished unit before they take their next units
 *                   together (1 = every lane at once, as up to round 2)
 *   "chunk_frames"  cap of the frames per launch pair of pbr_render / pbr_render_dof / pbr_render_adaptive (tests: several launch pairs)
 *   "face_normals"  0 = recompute the face normal on every hit (takes effect at the next pbr_upload_scene)
 *   "bvh_builder"   pbr_build_bvh: 0 clustering (default), 1 round 1's radix tree; "ploc_radius": its search radius
 *   "tune_log"      1 = the schedule tuner logs its launches to stderr
 *   "deal_order"    the queue's dealing order: 0 always spatial, 1 always cost classes, 2 always expensive last (once learnt), -1 by the render call's size
 *   "chain_layout"  the focus chain's table (pbr_render_dof): 0 frame-major planes (default), 1 a pixel slot's frames side by side
 *   "display_merge" pbr_display's histogram kernel: merge rounds per wave and group of 64 pixels ahead of the LDS adds, 0, 1, 2 or 4
 *                   (any other value: the default; csrc/pt_display.hpp).  The counts do not depend on it (tested)
 * Setting a knob rebuilds the plans and restarts the schedule tuner. */
int pbr_diag_set_knob( pbr_ctx* ctx, const char* name, int value );

/* Render with plan 0..6 (the order of pbr_diag_last_plan's *tuned: refill-lean, refill-wide, phased-lean, phased-wide,
 * phased-mid, refill-mid, phased-dual) from now on, without tuning; -1 hands the choice back to the tuner.  For the ranks of a
 * multi-GPU run: rank 0 tunes, broadcasts its *tuned, every rank pins it — all ranks then run the same schedule and
 * none is a straggler of the closing all-gather because its own timing noise picked a slower plan.  Survives
 * pbr_upload_scene / pbr_configure. */
int pbr_diag_pin_plan( pbr_ctx* ctx, int plan );

/* The dealing order of the work queue (csrc/pt_kernel.hpp, nextSlot).  The local tiles form a grid that is cut into 8 bands
 * of rows; band b's tiles are dealt in the order the stretch [band_first[b], band_first[b + 1]) of the table names them (local
 * tile indices; the table has one entry per local tile) — by four queue heads side by side, head s taking entries s, s + 4, ... of
 * the stretch.
 * Placement is for speed only: every (pixel, frame) unit is handed out exactly once in any order, images and counters
 * do not depend on it (tested).  get: which = 0 the spatial (or pinned) table, 1 the library's cost-classes table, 2 its
 * expensive-last table (PBR_ESTATE until they have been learnt); *count = entries, order[] filled when non-null.  set: with band_first = NULL `order` must hold,
 * per band, a permutation of that band's own tiles; with band_first[9] ANY partition of the local tiles into eight lists
 * (band_first[0] = 0, non-decreasing, band_first[8] = count; every tile once) — else PBR_EINVAL.  The table then stays in
 * force until pbr_configure (the library's own choice is off meanwhile); order = NULL: back to the library's choice. */
int pbr_diag_get_tile_order( pbr_ctx* ctx, int which, uint32_t* order, uint32_t capacity, uint32_t* count, uint32_t band_first[9] );
int pbr_diag_set_tile_order( pbr_ctx* ctx, const uint32_t* order, uint32_t count, const uint32_t* band_first );

/* The order the last render was dealt in: "spatial" — inside a band column by column —; "cost-classes" — per band eight
 * classes of falling cost, spatial inside a class: render calls of up to 128 Ki tiles x frames, of a shard (tile_world > 1) up
 * to 1 Mi —; "expensive-last" — per band its most expensive quarter last, spatial inside both parts: calls above 192 Ki (1 Mi) —,
 * the two once the library has learnt the
 * tiles' costs from a debug image (csrc/pbr_hip.hip, learnTileCosts); or "pinned" (pbr_diag_set_tile_order).  *learnt =
 * whether the cost orders exist.  Knob "deal_order": 0 always spatial, 1 always cost classes, 2 always expensive last (once
 * learnt), -1 by size. */
int pbr_diag_last_deal( pbr_ctx* ctx, char* name, size_t capacity, int* learnt );

/* How many frames of the configured size the schedule tuner wants to see before it settles (its launch lengths are
 * fixed in 1080p-frame equivalents, so a rank of an N-GPU run needs N times as many): a benchmark renders that many
 * before it starts its clock. */
int pbr_diag_tune_budget( pbr_ctx* ctx, uint32_t* frames );

/* The path-tracing launches of the last render: their summed duration (HIP events around each one)
 * and their number.  A multi-frame render is one launch unless its per-frame result buffer would
 * exceed 16 GiB; pbr_last_kernel_ms covers the whole render, foldFrames launches included. */
int pbr_diag_last_trace( pbr_ctx* ctx, double* trace_ms, uint32_t* launches );

/* The focus chain of the last render (pbr_render_dof with a focus point: the pre-pass ahead of every path-tracing launch,
 * csrc/pt_chain.hpp): its summed duration, 0 for every other render.  pbr_diag_last_trace keeps meaning the path launches. */
int pbr_diag_last_focus_chain( pbr_ctx* ctx, double* ms );

/* The last pbr_render_adaptive: how many rounds it ran (= convergence tests of a tile that never stopped), the (pixel, frame)
 * units it traced — the sum over the local tiles of 64 x frames rendered; against 64 x tiles x max_frames that is the saving —
 * and the summed duration of its folds (foldFramesAdaptive, csrc/pt_adaptive.hpp).  pbr_diag_last_trace and pbr_last_kernel_ms
 * report its path-tracing launches and the whole call (the host's table building between rounds included).
 * PBR_ESTATE before the first adaptive call. */
int pbr_diag_last_adaptive( pbr_ctx* ctx, uint32_t* rounds, uint64_t* units_traced, double* fold_ms );

/* All 16 device counter slots: [0..3] = pbr_counters; [4..15] are written only by experiment
 * builds (-DPBR_LAB_HOOKS, lab/src/pt_lab_hooks.hpp) and stay 0 otherwise. */
int pbr_diag_raw_counters( pbr_ctx* ctx, uint64_t out[16] );

/* Loop-bound trips of the LAST render, recorded by a PBR_GUARD build ([0] unused since round 3, [1] path loop,
 * [2] traversal); all zero in a normal build.  A render in which a bounded loop gave up returns PBR_EDEVICE. */
int pbr_diag_guard_trips( pbr_ctx* ctx, uint32_t out[3] );

/* The last pbr_display: the device time of its histogram kernel (0 when it launched none) and of its map kernel;
 * pbr_last_kernel_ms is their sum.  PBR_EINVAL for a null argument. */
int pbr_diag_display_info( pbr_ctx* ctx, double* histogram_ms, double* map_ms );

#ifdef __cplusplus
}
#endif
#endif
