/*
 * pbr_hip.h — C ABI of the MI355X path-tracing core (libpbrhip.so).
 *
 * Drop-in boundary: this library replaces what the reference reaches through its `CL`
 * class (source/CL.h:20-83) as driven by `PathTracer` (source/PathTracer.cpp) — the OpenCL
 * context, the device buffers, the JIT-compiled `pathTracing` kernel
 * (source/opencl/pathtracing.cl:207-334) and the per-frame launch.  `CL` is not a stable
 * plugin ABI (cl_mem / cl_kernel leak through every signature and kernel constants travel
 * as source-text substitutions), so the entry points mirror the reference's CALL SEQUENCE;
 * each one names the reference call it stands for.  Plain pointers and sizes only.
 *
 * Conventions
 *  - every function returns 0 on success, a negative PBR_E* code otherwise;
 *    pbr_last_error( ctx ) holds the message.  Nothing calls exit() (the reference does:
 *    source/CL.cpp:78,210,349,442,524,541,565).
 *  - inputs are borrowed for the duration of the call and copied to the device
 *    (CL_MEM_COPY_HOST_PTR semantics, source/CL.h:26-33); outputs are copied into
 *    caller-provided buffers (source/CL.cpp:581-594).
 *  - one context = one HIP device + one stream; calls on a context are synchronous and not
 *    re-entrant; separate contexts may be driven from separate threads / processes.
 *  - there is NO CPU fallback: without a usable HIP device pbr_create fails.
 */
#ifndef PBR_HIP_H
#define PBR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The layout of this header's structs and the meaning of its calls, as a number: bumped whenever a struct grows or an
 * entry point changes (round 5 grew pbr_config from 60 to 68 bytes; version 7 added pbr_render_dof, version 8 pbr_render_adaptive,
 * version 9 pbr_update_vertices and pbr_read_bvh, version 10 pbr_read_variance and pbr_denoise_guided,
 * version 11 pbr_denoise_temporal and pbr_temporal_reset, version 12 pbr_temporal_track_motion and pbr_read_temporal_motion,
 * version 13 pbr_refit_ordered_walk, version 14 pbr_update_geometry, version 15 pbr_set_parts, pbr_update_transforms and
 * pbr_read_geometry, version 16 pbr_set_skin and pbr_update_skin,
 * version 17 pbr_set_morph, pbr_update_morph and pbr_update_pose, version 18 pbr_update_skin_dq, pbr_update_pose_dq and
 * pbr_dual_quats_from_matrices, version 19 pbr_display and pbr_display_reset).  A caller that loads the library at run time — or
 * links a libpbrhip.so it did not build — compares pbr_abi_version() with the PBR_ABI_VERSION it was compiled against
 * BEFORE it hands the library a struct: pbr_configure reads sizeof( pbr_config ) bytes of ITS version. */
#define PBR_ABI_VERSION 19
uint32_t pbr_abi_version( void );

#define PBR_OK 0
#define PBR_EINVAL (-1)   /* bad argument / scene fails validation */
#define PBR_EDEVICE (-2)  /* HIP error (message has the HIP error string) */
#define PBR_ESTATE (-3)   /* call sequence violated (e.g. render before upload/configure) */

typedef struct pbr_ctx pbr_ctx;

/* ---- wire formats: the reference's host structs, bit for bit (source/PathTracer.h:25-73) */

typedef struct { float x, y, z, w; } pbr_float4;
typedef struct { uint32_t x, y, z, w; } pbr_uint4;

/* camera_cl, PathTracer.h:25-32 (cl_float3 occupies 16 bytes) — 80 bytes */
typedef struct {
	pbr_float4 eye, w, u, v;
	int32_t focusPoint[2];   /* (-1,-1): no depth of field */
	float lense[2];          /* focal length, aperture */
} pbr_camera;

/* bvhNode_cl, PathTracer.h:69-72 — 32 bytes.  bbMin.w: first face index or -1 (inner);
 * bbMax.w: second face index or -1 (leaf) / miss link or -1 (inner). */
typedef struct { pbr_float4 bbMin, bbMax; } pbr_bvh_node;

/* light_cl, PathTracer.h:39-43 — 48 bytes.  data.x: 1 point, 2 orb; data.y: orb radius */
typedef struct { pbr_float4 pos, rgb, data; } pbr_light;

/* material_schlick_rgb, PathTracer.h:45-54 — 48 bytes; data = d, Ni, p, rough */
typedef struct { float data[4]; pbr_float4 rgbDiff, rgbSpec; } pbr_material_schlick;

/* material_shirley_ashikhmin_rgb, PathTracer.h:56-65 — 64 bytes; data = d, Ni, nu, nv, Rs, Rd, -, - */
typedef struct { float data[8]; pbr_float4 rgbDiff, rgbSpec; } pbr_material_sa;

/* The seven arrays PathTracer::initOpenCLBuffers uploads (PathTracer.cpp:357-380 vertices /
 * normals, :238-347 bvh / facesV / facesN, :435-519 materials, :387-428 lights). */
typedef struct {
	const pbr_bvh_node* bvh;      uint32_t num_nodes;       /* -> #BVH_NUM_NODES# */
	const pbr_uint4* facesV;      /* {v0, v1, v2, material}, leaf order */
	const pbr_uint4* facesN;      /* may be NULL (only Phong tessellation reads it) */
	uint32_t num_faces;
	const pbr_float4* vertices;   uint32_t num_vertices;
	const pbr_float4* normals;    uint32_t num_normals;     /* may be NULL / 0 */
	const void* materials;        uint32_t num_materials;   /* pbr_material_schlick[] if brdf == 0, pbr_material_sa[] if 1 */
	uint32_t brdf;                /* which material layout `materials` uses */
	const pbr_light* lights;      uint32_t num_lights;      /* -> #NUM_LIGHTS#; lights may be NULL when 0 */
} pbr_scene_desc;

/* The constants CL::setValues / setReplacement bake into the kernel source
 * (source/CL.cpp:637-678, PathTracer.cpp:210,338,472,515). */
typedef struct {
	uint32_t width, height;       /* IMG_WIDTH, IMG_HEIGHT; multiples of 8 (opencl.localgroupsize) */
	uint32_t brdf;                /* BRDF: 0 Schlick, 1 Shirley-Ashikhmin; must match the uploaded materials */
	uint32_t shadow_rays;         /* SHADOW_RAYS */
	uint32_t max_depth;           /* MAX_DEPTH */
	uint32_t max_added_depth;     /* MAX_ADDED_DEPTH */
	uint32_t samples;             /* SAMPLES (paths per pixel per frame) */
	float anti_aliasing;          /* ANTI_ALIASING */
	float phong_tessellation;     /* PHONGTESS_ALPHA; > 0 = PHONGTESS on (pt_phongtess.cl; needs facesN / normals in the scene), 0 = flat triangles.
	                               * Phong tessellation pins its own schedule: the lock-step kernel in the 128-register budget is the only one built
	                               * with the patch intersection (the cubic solve spills in every budget, least in this one, and a state machine that parks lanes on
	                               * leaves would have to carry the patch normal through the park) — the tuner and pbr_diag_pin_plan do not apply. */
	float sky_light[4];           /* SKY_LIGHT */
	/* Tile sharding (not in the reference, which is single-device): this context renders the
	 * 8x8-pixel tiles whose position p in the dealing order has p % tile_world == tile_rank, where tile (tx, ty) has
	 * p = ty * tilesX + ( tx + 5 * ty ) % tilesX (row-major with row ty rotated by 5 * ty columns: plain row-major
	 * order would hand a rank whole tile columns whenever tilesX is a multiple of tile_world, and columns do not cost
	 * the same).  Local tile j of a rank is the tile at p = j * tile_world + tile_rank.  1 / 0 = everything, p = tile. */
	uint32_t tile_world, tile_rank;
	/* Two opt-in modes that are NOT reference constants; 0 / 0 (the value-initialised struct) is the reference's behaviour.
	 * traversal  PBR_WALK_REFERENCE (0): the reference's walk — a hit continues at index + 1 (pt_bvh.cl:102,112), the
	 *            child with the bigger surface area first whatever the ray (accelstructures/BVH.cpp:335-343).
	 *            PBR_WALK_SIX_ORDERS (1): the same flat tree, same boxes, leaves and per-visit arithmetic, but the children
	 *            of every container are visited in the order of their box centres along the ray direction's dominant axis
	 *            (six successor sets, chosen once per ray; still stackless).  Closest hits are the same faces at the same t
	 *            except where two faces tie exactly; the node / face-test counters and the debug image are this walk's own.
	 *            PBR_WALK_EIGHT_ORDERS (2): likewise with eight successor sets, one per sign octant of the ray direction;
	 *            every container orders its children along ITS axis (the one their centres spread furthest on).
	 *            Both cost node memory (6 / 8 streams of 32-byte records instead of one; they are built by the pbr_configure /
	 *            pbr_upload_scene call that completes "scene + such a mode" — which is also the call that fails when a tree
	 *            cannot be walked that way — and freed when another traversal is configured) and ~40 bytes of host memory
	 *            per node for the copy of the tree they are built from (kept from every upload).
	 *            PBR_WALK_EIGHT_ORDERS_COMPACT (3, round 6): the eight-order walk — same visits, same counters, same hits —
	 *            over ONE 64-byte record per node shared by the eight orders (two hit candidates picked by a sign bit,
	 *            eight `next` words): twice the reference stream's node memory instead of eight times, and scenes up to
	 *            the wire format's own 2^24 nodes (eight streams: 8.3 M); one more 4-byte load and five more vector
	 *            instructions per visit.
	 * arith      PBR_ARITH_EXACT (0): every builtin has one correctly rounded / fixed definition.
	 *            PBR_ARITH_NATIVE (1): what the reference asks its device for — native_sin / native_cos / native_tan /
	 *            native_recip / native_divide / native_sqrt (pt_utils.cl:39-44, pt_brdf.cl:306-321, pt_intersect.cl:104,
	 *            pt_bvh.cl:83) as the gfx950 instructions, pow through v_log_f32 / v_exp_f32.  Images then agree with the
	 *            exact mode statistically, not bit for bit. */
	uint32_t traversal;
	uint32_t arith;
} pbr_config;

#define PBR_WALK_REFERENCE 0u
#define PBR_WALK_SIX_ORDERS 1u
#define PBR_WALK_EIGHT_ORDERS 2u
#define PBR_WALK_EIGHT_ORDERS_COMPACT 3u
#define PBR_ARITH_EXACT 0u
#define PBR_ARITH_NATIVE 1u

/* Traversal counters (the reference's debugColor.y / .x, pt_bvh.cl:89,23, as exact integers,
 * plus shaded hits and camera paths) summed over everything rendered since the last reset. */
typedef struct { uint64_t nodes, tris, hits, paths; } pbr_counters;

/* Which modes this build of the library carries: 1 if every plan's kernels for ( traversal, arith ) were linked in, 0 if not
 * (a build may leave a mode's translation units out), -1 for values that are no mode.  No device
 * is needed.  pbr_configure refuses (PBR_ESTATE, with a message) a mode whose kernels were not built. */
int pbr_mode_built( uint32_t traversal, uint32_t arith );

/* new CL() — platform / device / context / profiling queue (source/CL.cpp:10-24). */
int pbr_create( int device, pbr_ctx** out );
/* ~CL() (source/CL.cpp:30-52) */
void pbr_destroy( pbr_ctx* ctx );
const char* pbr_last_error( const pbr_ctx* ctx );

/* CL::createBuffer x 7 (PathTracer.cpp:357-519).  Validates every index the kernel will
 * follow (links, face, vertex and material indices — the reference reads out of bounds for
 * material -1, ObjParser.cpp:140,192) and re-lays the arrays out for CDNA4. */
int pbr_upload_scene( pbr_ctx* ctx, const pbr_scene_desc* scene );
/* The checks of pbr_upload_scene alone, without a context or a device (a host-side loader can vet a foreign BVH
 * before it goes anywhere near a GPU): array sizes, every node's face / link words — miss links must be integers in
 * [-1, N) that point FORWARD (the stackless walk of pt_bvh.cl:96-117 keeps no visited set; a backward link would make
 * it circle forever) — leaf pairs k, k + 1, the last node a leaf, vertex and material indices of every face.
 * Returns PBR_OK or PBR_EINVAL with the reason in message[capacity]. */
int pbr_validate_scene( const pbr_scene_desc* scene, char* message, size_t capacity );

/* Moving geometry (not in the reference, whose scene is static): replaces the vertex positions of the uploaded scene and
 * rebuilds ON THE DEVICE everything that was derived from them — the face records {a, b - a, c - a, material}, the per-face
 * normals (unless the "face_normals" knob was 0 at the upload) and every node's box (a REFIT: the tree's links, the faces,
 * materials and lights are kept).  `vertices` is host memory, borrowed for the call; num_vertices must be the upload's.
 * pbr_last_kernel_ms then reports the device time of the update's kernels; the copy of the vertices to the device is NOT in
 * it (pbr_diag_refit_info, pbr_hip_diag.h, reports it next to it).
 * The boxes, operation by operation, per component in binary32 — reproducible to the bit:
 *   leaf       start from corner a of its first face; fold in b, c, then the second face's a, b, c if there is one, with
 *              lo = ( v < lo ) ? v : lo and hi = ( v > hi ) ? v : hi;
 *   container  (node 0 included) the same fold over its children's boxes in depth-first child order, starting from the first
 *              child's box; the children of i are c0 = i + 1, c1 = end( c0 ), ... below end( i ) (there can be more than two);
 *   the .w words are unchanged.
 * These are tight boxes of the flat triangles, NOT the reference builder's (MathHelp.cpp:260-309 thickens a triangle's box
 * for Phong tessellation): an update with the very vertices that were uploaded may change boxes, and — through tNear,
 * pt_intersect.cl:96-97 — bits of t.  THE CONTRACT is equality with a fresh upload, not with the state before: after
 * pbr_upload_scene( S ) and pbr_update_vertices( V' ) every call (pbr_render*, pbr_render_frame, pbr_diag_trace,
 * pbr_denoise, the counters, the debug image) gives bit for bit what it gives after pbr_upload_scene( S' ), S' = S with the
 * vertices V' and the nodes pbr_read_bvh returns.  Only speed may differ: the ranking of the nodes staged in LDS, the schedule
 * tuner's kept plan, the learnt tile costs and the dealing orders stay from before the update (pbr_diag_set_knob or a new
 * upload re-tunes).  The accumulated image is not touched: resetting it is the caller's business, as after a camera move.
 * Refusals, each leaving the context unchanged:
 *   PBR_ESTATE  no scene; a tree that is not properly nested (pbr_validate_scene accepts any forward link, a refit needs the
 *               children of every container to tile [i + 1, end( i )) exactly, and no container without a child — decided at
 *               the upload, the reason is in the message); a ray-ordered traversal (traversal != 0) is configured (its streams
 *               carry child orders built from the old box centres: configure traversal 0, update, configure the ordered walk
 *               again — it is then built from the refitted boxes, bit-identical to a fresh upload of S' + the same
 *               pbr_configure) unless pbr_refit_ordered_walk is on, see below; phong_tessellation > 0 is configured.
 *   PBR_EINVAL  a null pointer, num_vertices other than the upload's, a coordinate that is not finite (checked on the host).
 * After an update pbr_configure refuses phong_tessellation > 0 (PBR_ESTATE) until the next pbr_upload_scene: tight boxes
 * would clip the patches, and the patches' corners are not updated.  pbr_update_geometry (below, ABI version 14) is the update
 * that moves the patches too and works while Phong tessellation is configured. */
int pbr_update_vertices( pbr_ctx* ctx, const pbr_float4* vertices, uint32_t num_vertices );
/* A REFIT UNDER A RAY-ORDERED WALK (ABI version 13).  pbr_refit_ordered_walk( ctx, 1 ) makes pbr_update_vertices succeed while
 * traversal 1, 2 or 3 is configured: behind the refit above it rebuilds, on the device and in place, the records of the
 * configured layout — every record's box, every container's hit word(s) and the axis bit of the compact record, every `next`
 * word of every order, the place of every cold record in its order's depth-first sequence, and the 32-byte header of eight
 * first references.  The flag is per context, 0 after pbr_create, needs no scene and survives pbr_configure and
 * pbr_upload_scene; PBR_EINVAL for a null context, PBR_ESTATE for an unusable one.  With the flag off nothing changes (the
 * refusal above, bit for bit); with it on and traversal 0 configured the call is the one above.  Every other refusal stays, in
 * the same order, and leaves the context and the streams as they were.
 * THE CONTRACT.  After pbr_upload_scene( S ), pbr_configure( t ) and pbr_update_vertices( V' ) with the flag on, the
 * configured layout's device buffer is BYTE FOR BYTE the one the three-call sequence leaves — pbr_configure( traversal 0 ),
 * pbr_update_vertices( V' ), pbr_configure( t ) — on a context that uploaded the same S: the records of the tree with the
 * refitted boxes pbr_read_bvh returns under the hot-node ranking OF THE UPLOAD (the ranking stays stale, as it does for the
 * reference-order stream: it is only speed), the number of staged records and the header with them.  Hence every call
 * (pbr_render*, pbr_render_frame, pbr_diag_trace, the counters, the debug image, pbr_denoise*) gives bit for bit what it gives
 * after a fresh upload of S' and the same pbr_configure.  pbr_diag_read_walk (pbr_hip_diag.h) reads the buffer back.
 * The orders, operation by operation: a child's key on an axis is bbMin + bbMax of that axis, one binary32 addition of the
 * refitted box words; schemes 2 and 3 sort a container's children on its own axis, the first of x, y, z whose hi - lo of the
 * children's keys (lo = ( k < lo ) ? k : lo, hi = ( k > hi ) ? k : hi, from +inf / -inf) is strictly greater than the widest
 * so far, starting from -1; scheme 1's order k sorts on axis k / 2.  The sort is an insertion sort of the depth-first child list
 * with strict compares: equal keys keep depth-first order ascending AND descending.
 * No node, box or record travels to the host (the 32 bytes of the header do: the context keeps the first references), and
 * nothing is allocated or freed per call: the working tables — some 90 bytes per node for layouts 1 and 2, 60 for layout 3
 * (pbr_diag_relink_info) — are allocated by the FIRST such update after the layout's records were built, and freed with them (another
 * layout configured, pbr_configure( traversal 0 ) followed by an update, a new upload).  pbr_last_kernel_ms includes the
 * re-link's kernels; pbr_diag_relink_info reports their share.  Configuring another ordered layout afterwards builds its
 * records on the host from the refitted tree, as before. */
int pbr_refit_ordered_walk( pbr_ctx* ctx, int on );
/* A REFIT UNDER PHONG TESSELLATION (ABI version 14).  pbr_update_geometry takes new vertex positions AND new vertex normals for
 * the uploaded scene and rebuilds on the device what pbr_update_vertices rebuilds — the face records, the per-face normals,
 * every node's box, the re-link of the configured ordered layout when pbr_refit_ordered_walk is on — and with them the Phong
 * patch records the patch intersection reads: per face six quads, the three corners, then the three vertex normals, gathered
 * through facesV / facesN, each with .w = 0.  `vertices` and `normals` are host memory, borrowed for the call.
 *   normals == NULL with num_normals == 0   positions only: the normals stay the ones the context holds (the upload's, or
 *                                           those of the last pbr_update_geometry that brought some);
 *   otherwise                               num_normals must be the upload's count.
 * The boxes are built with alpha = the configured phong_tessellation (0 for a context that is not configured), so the call
 * succeeds WHILE Phong tessellation is configured, where pbr_update_vertices refuses.
 * THE FACE BOX, operation by operation in binary32, none fused (it is the reference builder's thickened box, MathHelp.cpp:250-310
 * and :325-378, with the refit's fold); p1, p2, p3 are the face's corners a, b, c and n1, n2, n3 its vertex normals:
 *   lo = hi = p1; fold p2, then p3, with lo = ( v < lo ) ? v : lo and hi = ( v > hi ) ? v : hi per component;
 *   if alpha > 0 and the three normals are NOT EQUAL — t = ( n1 - n2 ) + ( n2 - n3 ), any fabsf( t.k ) > 0.000001f — fold, in
 *   this order, the three raised corners p_k + thickness * ng, k = 1, 2, 3, and the nine edge points phongPoint( u, v ) for
 *   ( u, v ) = ( 0, .5 ) ( .5, 0 ) ( .5, .5 ) ( .25, .75 ) ( .75, .25 ) ( .25, 0 ) ( .75, 0 ) ( 0, .25 ) ( 0, .75 ), where
 *     dot( a, b ) = ( a.x*b.x + a.y*b.y ) + a.z*b.z      normalize( a ) = a * ( 1.0f / sqrtf( dot( a, a ) ) )
 *     cross( a, b ) = { a.y*b.z - b.y*a.z, a.z*b.x - b.z*a.x, a.x*b.y - b.x*a.y }
 *     e12 = p2 - p1, e13 = p3 - p1, e23 = p3 - p2, e31 = p1 - p3
 *     c12 = alpha * ( dot( n2, e12 ) * n2 - dot( n1, e12 ) * n1 )
 *     c23 = alpha * ( dot( n3, e23 ) * n3 - dot( n2, e23 ) * n2 )
 *     c31 = alpha * ( dot( n1, e31 ) * n1 - dot( n3, e31 ) * n3 )
 *     ng = normalize( cross( e12, e13 ) )
 *     m = dot( ng, ( c12 - c23 ) - c31 )
 *     k = 1.0f / ( ( 4.0f * dot( ng, c23 ) ) * dot( ng, c31 ) - m * m )
 *     u = k * ( ( 2.0f * dot( ng, c23 ) ) * dot( ng, c31 + e31 ) + dot( ng, c23 - e23 ) * m )
 *     v = k * ( ( 2.0f * dot( ng, c31 ) ) * dot( ng, c23 - e23 ) + dot( ng, c31 + e31 ) * m )
 *     u = ( u < 0 || u > 1 ) ? 0 : u, likewise v
 *     thickness = dot( ng, phongPoint( u, v ) - p1 )
 *     phongPoint( u, v ):  w = ( 1.0f - u ) - v;  bary = ( p1 * u + p2 * v ) + p3 * w;
 *                          onPlane( q, p, n ) = q - dot( q - p, n ) * n;
 *                          tess = ( u * onPlane( bary, p1, n1 ) + v * onPlane( bary, p2, n2 ) ) + w * onPlane( bary, p3, n3 );
 *                          the point is ( 1.0f - alpha ) * bary + alpha * tess
 *   a vector times a scalar is three multiplications; `/` and sqrtf are correctly rounded.
 * A NaN point never enters the fold, because both compares are false (a face without area has ng = NaN: its box is the tight
 * one; an infinite k gives NaN or 0 for u and v); corners are finite by the host's check, so no box word is ever NaN.
 *   leaf       ONE running fold: its first face's twelve-or-three points, then its second face's if there is one;
 *   container  exactly as pbr_update_vertices; the .w words are unchanged.
 * With alpha = 0 every box is, bit for bit, pbr_update_vertices's.
 * THE CONTRACT is the refit's: after pbr_upload_scene( S ), pbr_configure( c ) and pbr_update_geometry( V', N' ) every call
 * (pbr_render*, pbr_render_frame, pbr_diag_trace, the counters, the debug image, pbr_denoise*) gives bit for bit what it gives
 * after pbr_upload_scene( S' ) and pbr_configure( c ), S' = S with V', N' and the nodes pbr_read_bvh returns — Phong
 * tessellation included, in all four traversals.  What stays stale stays stale: the hot-node ranking, the tuner's plan, the tile
 * costs and the dealing orders.  The temporal history is treated as by pbr_update_vertices: dropped, or H kept under
 * pbr_temporal_track_motion (the motion path stays NOT COVERED under Phong tessellation).
 * Refusals, each leaving the context unchanged:
 *   PBR_ESTATE  no scene; a tree that is not properly nested; a ray-ordered traversal without pbr_refit_ordered_walk (the
 *               refit's own, in its order); `normals` given for a scene that was uploaded without usable vertex normals.
 *   PBR_EINVAL  a null context; null `vertices`; a count other than the upload's; `normals` and num_normals disagreeing about
 *               NULL / 0; a position or normal coordinate that is not finite.
 * THE STATE RULE of pbr_configure: after any update it refuses phong_tessellation > 0 (PBR_ESTATE) unless the most recent
 * successful update was a pbr_update_geometry AND the alpha of that update equals cfg->phong_tessellation, compared as floats.
 * A later pbr_update_vertices brings the refusal back (it leaves the patches stale and the boxes tight); a new upload clears it.
 * Configuring phong_tessellation = 0 over thick boxes is always allowed: thick boxes are conservative, and the contract covers
 * them through pbr_read_bvh.  pbr_update_vertices itself is unchanged, its refusal under Phong tessellation included.
 * Nothing is allocated per call: the device tables — 16 bytes per face (its normal indices), 16 per normal, 24 per face (its
 * thick box, written by the patch kernel and read by the leaf step one launch later) — are made by the FIRST pbr_update_geometry
 * after an upload from a host copy the upload keeps, and freed with the scene (pbr_diag_patch_refit_info, pbr_hip_diag.h). */
int pbr_update_geometry( pbr_ctx* ctx, const pbr_float4* vertices, uint32_t num_vertices,
                         const pbr_float4* normals, uint32_t num_normals );
/* RIGID OR AFFINE MOTION PER PART, COMPUTED ON THE DEVICE (ABI version 15).  The motion callers mostly have is a few matrices —
 * doors, wheels, props, a turntable —, not new vertices: pbr_set_parts says once which part every vertex (and every vertex
 * normal) belongs to and captures the REST POSE, pbr_update_transforms then takes num_parts matrices, computes V' and N' on
 * the device from the rest pose and does exactly what pbr_update_geometry( V', N' ) does.  Only the matrices travel.
 *
 * pbr_set_parts: vertex_part[num_vertices], each < num_parts, num_vertices the upload's count; normal_part likewise for the
 * vertex normals —
 *   normal_part == NULL with num_normals == 0   the normals are never transformed (an update then is a
 *                                               pbr_update_geometry( V', NULL, 0 ));
 *   otherwise                                   num_normals must be the upload's count, and the scene must have usable vertex
 *                                               normals (pbr_update_geometry's condition for new normals).
 * The call captures the rest pose: the vertex positions as they are on the device NOW, copied device to device, and with normal
 * parts the normals the context holds now (the upload's, or those of the last pbr_update_geometry that brought some).
 * num_parts == 0 with both pointers NULL drops the parts and frees their buffers; a second call replaces parts and rest pose;
 * pbr_upload_scene drops them; pbr_configure, pbr_update_vertices and pbr_update_geometry leave them alone — a later transform
 * starts again from the rest pose, not from what those calls wrote.
 * Refusals, each leaving the context and the parts that were set unchanged:
 *   PBR_ESTATE  no scene; normal parts for a scene without usable vertex normals.
 *   PBR_EINVAL  a null context; null vertex_part; a count other than the upload's; normal_part and num_normals disagreeing about
 *               NULL / 0; num_parts == 0 with a pointer; an index >= num_parts (the message names the first one).
 * ALL allocation happens in this call: 16 + 4 bytes per vertex (rest position, part index), the same per normal if normal parts
 * are given, one 16-byte-per-vertex staging buffer, 96 bytes per part (its record) and a 4-byte flag word
 * (pbr_diag_transform_info, pbr_hip_diag.h) — and pbr_update_geometry's tables if the scene has patches and no update made them
 * yet.  pbr_update_transforms allocates nothing.
 *
 * pbr_update_transforms: `matrices` is host memory, borrowed for the call, num_parts x 12 floats.  Part k's matrix is row-major
 * 3 x 4: rows r = 0, 1, 2 are m[4r .. 4r+3], a_r is the first three words of row r, m[4r+3] the translation.  V' and N' are
 * computed from the REST POSE, never from the current positions: it is not cumulative, there is no drift.
 * THE DEFINITION, operation by operation in binary32, none fused; dot and cross are pbr_update_geometry's above, `/` and sqrtf
 * are correctly rounded.
 *   per part, once, on the host:
 *     c0 = cross( a1, a2 ), c1 = cross( a2, a0 ), c2 = cross( a0, a1 ), det = dot( a0, c0 );
 *     if det < 0 every word of c0, c1, c2 is negated.  The nine words travel with the twelve.
 *   position p of part k:
 *     p'.x = ( ( m0*p.x + m1*p.y ) + m2*p.z ) + m3, rows 1 and 2 likewise; p'.w = p.w bit for bit
 *   normal n of part k:
 *     q.r = dot( c_r, n ), d = dot( q, q );
 *     if d > 0 and d < inf   n'.xyz = q * ( 1.0f / sqrtf( d ) ) (three multiplications)
 *     else                   n'.xyz = n.xyz bit for bit;
 *     n'.w = n.w.  So no normal word is ever NaN.
 *   AN IDENTITY PART — its twelve words compare equal, as floats, to the identity — copies its rest positions and normals bit
 *   for bit: -0 stays -0 and a unit normal does not move by an ulp, so unmoved parts ARE unmoved for pbr_denoise_temporal's
 *   UNMOVED test and for a caller's diff.
 * THE CONTRACT.  After pbr_set_parts and pbr_update_transforms( M ) every call gives bit for bit what it gives after
 * pbr_update_geometry( V', N' ) on a context in the same state — pbr_render*, pbr_render_frame, pbr_diag_trace, the counters,
 * the debug image, pbr_denoise*, pbr_read_bvh, pbr_diag_read_patches, pbr_diag_read_walk — and hence what a fresh upload of S'
 * gives; in all four traversals (with pbr_refit_ordered_walk for the ordered ones) and under Phong tessellation.  All state
 * follows pbr_update_geometry's rules unchanged: pbr_configure's state rule (the call counts as a pbr_update_geometry with the
 * alpha it ran under), pbr_diag_patch_refit_info, pbr_diag_refit_info (its upload_ms now times the asynchronous copy of the part
 * records from pinned memory) and pbr_diag_relink_info, the temporal history (H is taken before the vertices change;
 * pbr_temporal_track_motion works through it), and what stays stale.  pbr_last_kernel_ms covers the whole update, the transform
 * kernels and the read-back of the flag word between them included.
 * Refusals, each leaving the context, the vertices, the normals and the tree exactly as they were:
 *   PBR_EINVAL  a null context;
 *   PBR_ESTATE  no parts set (the message names pbr_set_parts; a new upload drops them);
 *   PBR_EINVAL  null `matrices`, or num_parts other than the set one; a matrix word that is not finite; a det that is 0 or not
 *               finite, or a c word that is not finite (the message names the part);
 *   then pbr_update_geometry's own refusals, in its order;
 *   PBR_EINVAL  a coordinate of V' that is not finite — finite matrices can overflow.  This is found ON THE DEVICE, because the
 *               host never sees V': the transform kernel writes V' to the staging buffer and raises a flag word, the host reads
 *               its 4 bytes and only then makes the staging buffer the context's vertices (the two pointers are swapped).  The
 *               normals cannot fail and are written after that check.
 * OUT OF SCOPE: pbr_multi.h (every rank would take the same matrices: call this on each rank's context), per-vertex skinning
 * and blend weights (not in these two calls: pbr_set_skin and pbr_update_skin below, ABI version 16, do that), topology changes. */
int pbr_set_parts( pbr_ctx* ctx, const uint32_t* vertex_part, uint32_t num_vertices, const uint32_t* normal_part, uint32_t num_normals,
                   uint32_t num_parts );
int pbr_update_transforms( pbr_ctx* ctx, const float* matrices, uint32_t num_parts );
/* BLEND-WEIGHT SKINNING, COMPUTED ON THE DEVICE (ABI version 16).  Characters, cloth rigs, bending pipes: every vertex (and every
 * vertex normal) follows up to PBR_SKIN_INFLUENCES bones, each with a weight.  pbr_set_skin says once which bones and weights and
 * captures the REST POSE, pbr_update_skin then takes num_bones matrices, blends them per element on the device, computes V' and
 * N' from the rest pose and does exactly what pbr_update_geometry( V', N' ) does.  Only the matrices travel.
 *
 * pbr_set_skin: vertex_bones[4*i + j] and vertex_weights[4*i + j] are slot j of vertex i, num_vertices the upload's count;
 * normal_bones / normal_weights likewise for the vertex normals, which have their own indices (facesN) —
 *   normal_bones == NULL, normal_weights == NULL, num_normals == 0   the normals are never transformed (an update then is a
 *                                                                     pbr_update_geometry( V', NULL, 0 ));
 *   otherwise                                                         num_normals must be the upload's count, and the scene
 *                                                                     must have usable vertex normals.
 * It mirrors pbr_set_parts in every rule that is not about weights.  The call captures the rest pose: the vertex positions as
 * they are on the device NOW, copied device to device, and with normal influences the normals the context holds now.
 * num_bones == 0 with all four pointers NULL drops the skin and frees its buffers; a second call replaces the skin and the rest
 * pose; pbr_upload_scene drops the skin; pbr_configure and the other update calls leave it alone — a later skin update starts
 * again from the rest pose.  A skin and parts are independent: either, both or neither may be set, each has its own rest pose,
 * neither call touches the other's state.
 * THE WEIGHTS ARE USED AS GIVEN: they are not normalised and their sum is not checked.
 * Refusals, each leaving the context and any skin that was set exactly as it was:
 *   PBR_EINVAL  a null context;
 *   PBR_ESTATE  no scene;
 *   PBR_EINVAL  in this order: null vertex_bones or null vertex_weights; a count other than the upload's (num_vertices, or a
 *               num_normals that is neither 0 nor the upload's); the three normal arguments disagreeing about NULL / 0;
 *               num_bones == 0 with a pointer; a bone index >= num_bones in any slot, zero-weight slots included (the message
 *               names element and slot); a weight that is not finite or is < 0; an element whose four weights are all 0 (the
 *               message names it);
 *   PBR_ESTATE  normal influences for a scene without usable vertex normals.
 * ALL allocation happens in this call: the library repacks the caller's arrays into one 32-byte influence record per element
 * (four bones, then four weights); 16 + 16 + 32 bytes per vertex (rest position, staging position, influence record), 16 + 32
 * per normal if normal influences are given, 48 bytes per bone and a 4-byte flag word (pbr_diag_skin_info, pbr_hip_diag.h) —
 * and pbr_update_geometry's tables if the scene has patches and no update made them yet.  pbr_update_skin allocates nothing.
 *
 * pbr_update_skin: `matrices` is host memory, borrowed for the call, num_bones x 12 floats, row-major 3 x 4 in
 * pbr_update_transforms' layout.  V' and N' are computed from the REST POSE: it never accumulates.
 * THE DEFINITION, operation by operation in binary32, none fused; dot, cross, `/` and sqrtf are pbr_update_geometry's.
 *   slots     S = the slots j = 0..3 of the element whose weight compares unequal to 0, in slot order.  A slot with weight 0
 *             contributes nothing, not even a +0, so an unused slot may name any valid bone.
 *   blended matrix B, twelve words k:
 *             for the first slot s of S   B[k] = w_s * m_s[k];
 *             for each later slot s       B[k] = B[k] + w_s * m_s[k] — a product and then an addition.
 *   position  p' = transformPosition( B, p ): p'.x = ( ( B0*p.x + B1*p.y ) + B2*p.z ) + B3, rows 1 and 2 likewise; p'.w = p.w
 *             bit for bit.  It includes the identity rule: a B whose twelve words compare equal, as floats, to the identity
 *             copies the rest words bit for bit.
 *   normal    B comes from the normal's own influences; ( c, det ) = cofactors( B ): c0 = cross( a1, a2 ), c1 = cross( a2, a0 ),
 *             c2 = cross( a0, a1 ), det = dot( a0, c0 ), every word negated if det < 0; n' = transformNormal( c, isIdentity( B ), n )
 *             as pbr_update_transforms defines it.  So a d that is 0, infinite or NaN copies the rest normal: a singular blend is
 *             legal and no normal word is ever NaN.
 * TWO PROPERTIES that follow, and that tests rest on:
 *   1. ONE-HOT SKIN EQUALS THE RIGID CALL.  An element with exactly one non-zero weight, equal to 1.0f, has B equal to that
 *      bone's matrix bit for bit (1.0f * x is x, -0 stays -0); its position and normal are bit for bit pbr_update_transforms'
 *      for a part with that matrix.
 *   2. UNMOVED ELEMENTS STAY UNMOVED.  Weights 1/2 + 1/2, 1/4 + 3/4 and the like of identity bones give an identity B; such an
 *      element is UNMOVED for pbr_denoise_temporal.  Weights that are not dyadic may or may not sum to 1.0f: that is NOT
 *      PROMISED.
 * THE CONTRACT.  After pbr_set_skin and pbr_update_skin( M ) every call gives bit for bit what it gives after
 * pbr_update_geometry( V', N' ) on a context in the same state, and hence what a fresh upload of the moved scene gives; in all
 * four traversals (with pbr_refit_ordered_walk for the ordered ones) and under Phong tessellation.  All state follows
 * pbr_update_geometry's rules: pbr_configure's state rule, pbr_diag_refit_info, pbr_diag_patch_refit_info and
 * pbr_diag_relink_info, the temporal history (H is taken before the vertices change; pbr_temporal_track_motion works through
 * it).  After a skin update pbr_diag_transform_info's last_update is 0; after a transform update the skin's last_update is 0.
 * Refusals, each leaving the context, the vertices, the normals and the tree exactly as they were:
 *   PBR_EINVAL  a null context;
 *   PBR_ESTATE  no skin set (the message names pbr_set_skin; a new upload drops it);
 *   PBR_EINVAL  null `matrices`; num_bones other than the set one; a matrix word that is not finite (the message names bone and
 *               word).  Bones are NOT checked for a zero determinant: the definition handles a singular B;
 *   then pbr_update_geometry's own refusals, in its order;
 *   PBR_EINVAL  a coordinate of V' that is not finite.  This is found ON THE DEVICE with pbr_update_transforms' mechanism: the
 *               kernel writes V' to the staging buffer and raises a flag word, the host reads 4 bytes, only then the pointers
 *               are swapped, and the normals are written after that check.
 * OUT OF SCOPE: more than four influences, dual-quaternion skinning, morph targets, pbr_multi.h, topology changes, and any
 * rebuild of a tree that large deformations have degraded — the refit's boxes remain what pbr_read_bvh shows.  (Morph
 * targets came with ABI version 17, in calls of their own: pbr_set_morph, pbr_update_morph and pbr_update_pose below.) */
#define PBR_SKIN_INFLUENCES 4
int pbr_set_skin( pbr_ctx* ctx, const uint32_t* vertex_bones, const float* vertex_weights, uint32_t num_vertices,
                  const uint32_t* normal_bones, const float* normal_weights, uint32_t num_normals, uint32_t num_bones );
int pbr_update_skin( pbr_ctx* ctx, const float* matrices, uint32_t num_bones );
/* MORPH TARGETS (BLEND SHAPES), COMPUTED ON THE DEVICE (ABI version 17).  Faces, muscle correctives, cloth caches: sparse per-vertex
 * (and per-normal) deltas, each target scaled by one weight per update, applied BEFORE the skin.  pbr_set_morph says once which
 * deltas and captures the REST POSE, pbr_update_morph then takes num_targets weights, computes V' and N' from the rest pose on
 * the device and does exactly what pbr_update_geometry( V', N' ) does; pbr_update_pose takes the weights and the matrices of the
 * skin that is set (pbr_set_skin) and is, bit for bit, the skin of the morphed rest pose.  Only weights and matrices travel.
 *
 * pbr_set_morph: sparse targets, target-major as exporters give them.  Target t owns entries vertex_first[t] ..
 * vertex_first[t+1]-1 (vertex_first has num_targets + 1 words); entry e is the element index vertex_index[e] and the delta quad
 * vertex_delta[e] (x, y, z used, w ignored and not checked).  normal_first / normal_index / normal_delta likewise for the vertex
 * normals, which have their own indices (facesN) — all three NULL: the normals are never morphed (an update then is a
 * pbr_update_geometry( V', NULL, 0 )); otherwise the scene must have usable vertex normals.  Empty targets and targets that touch
 * every element are both legal.  The call captures the rest pose as pbr_set_skin does: the vertex positions as they are on the
 * device NOW, copied device to device, and with normal targets the normals the context holds now.  num_targets == 0 with all six
 * pointers NULL drops the morph and frees its buffers; a second call replaces the morph and the rest pose; pbr_upload_scene
 * drops the morph; pbr_configure and the other update calls leave it alone.  A morph, a skin and parts are independent: each has
 * its own rest pose, no set call touches another's state.
 * Refusals, each checked before the device is touched and leaving the context and any morph that was set exactly as it was:
 *   PBR_EINVAL  a null context;
 *   PBR_ESTATE  no scene;
 *   PBR_EINVAL  in this order, within one rule the vertex lists before the normal lists: num_targets == 0 with a pointer; a null
 *               vertex_first, vertex_index or vertex_delta; the three normal pointers disagreeing about NULL; first[0] != 0 or a
 *               `first` array that decreases; an index >= the uploaded count; an index that occurs twice within one target; an
 *               x, y or z of a delta that is not finite (the messages name target and entry);
 *   PBR_ESTATE  normal targets for a scene without usable vertex normals.
 * ALL allocation happens in this call: the library transposes the lists into element-major runs — runFirst[count + 1] words and
 * one 16-byte entry { dx, dy, dz, target } per delta, an element's run in ascending target —; with V vertices, N normals, T
 * targets, Ev vertex entries and En normal entries it holds 16 V + 16 V + 4 ( V + 1 ) + 16 Ev bytes (rest position, staging
 * position, runs, entries), + 16 N + 4 ( N + 1 ) + 16 En with normal targets, + 4 T + 4 (weight table, flag word;
 * pbr_diag_morph_info, pbr_hip_diag.h) — and pbr_update_geometry's tables if the scene has patches and no update made them yet.
 * The update calls allocate nothing.
 *
 * pbr_update_morph: `weights` is host memory, borrowed for the call, num_targets floats.
 * THE DEFINITION, operation by operation in binary32, none fused; dot and sqrtf are pbr_update_geometry's.
 *   active    the targets whose weight compares unequal to 0, taken in ascending target index.  A target of weight 0
 *             contributes nothing, not even a +0.
 *   position  p' = p; for every entry ( t, d ) of the element with t active, in ascending t, for each of x, y, z:
 *             p'.c = p'.c + w_t * d.c — a product, then an addition.  p'.w = p.w bit for bit.  An element with no active entry
 *             is the rest quad bit for bit; in particular all weights 0 give the rest pose.
 *   normal    q = n + sum w_t d, accumulated the same way.  With no active entry n is copied.  Otherwise d = dot( q, q ); if
 *             !( d > 0 && d < inf ) n is copied, else n'.xyz = q * ( 1.0f / sqrtf( d ) ), n'.w = n.w — the tail of
 *             pbr_update_transforms' normal rule, so no normal word is ever NaN.
 *   weights   used as given: negative weights and weights above 1 are legal.
 * pbr_update_pose: per element skinPosition( B, p' ) and skinNormal( B, n' ) of pbr_update_skin's definition, p' and n' the
 * morphed rest quads above, B the element's blend of `matrices` (num_bones x 12 floats), its identity rule and its singular-blend
 * rule included.  Normals: morphed if the morph has normal targets, then skinned if the skin has normal influences; with
 * neither the context's normals stay.
 * NEVER CUMULATIVE: pbr_update_morph ignores a set skin, pbr_update_skin ignores a set morph; each of the three calls is a
 * function of the rest pose and its own arguments only.  pbr_update_pose( 0 weights, M ) equals pbr_update_skin( M );
 * pbr_update_pose( w, one-hot identity bones ) equals pbr_update_morph( w ).
 * THE CONTRACT is pbr_update_skin's: after the call every call gives bit for bit what it gives after pbr_update_geometry( V', N' ),
 * in all four traversals and under Phong tessellation; the temporal history hears of the update as it does for the skin.
 * Refusals, in this order, each before the device is touched and leaving the context, the vertices, the normals and the tree as
 * they were:
 *   PBR_EINVAL  a null context;
 *   PBR_ESTATE  no morph set (the message names pbr_set_morph; a new upload drops it);
 *   PBR_ESTATE  pbr_update_pose: no skin set;
 *   PBR_ESTATE  pbr_update_pose: skin and morph did not capture the same geometry — the context keeps a geometry generation,
 *               bumped by an upload and by every successful update of any kind; both set calls record it and they must agree;
 *   PBR_EINVAL  null `weights`; num_targets other than the set one; a weight that is not finite (the message names the target);
 *   PBR_EINVAL  pbr_update_pose: everything pbr_update_skin refuses about `matrices` and num_bones;
 *   then pbr_update_geometry's own refusals, in its order (a tree that is not nested, an ordered traversal without
 *   pbr_refit_ordered_walk, ...);
 *   PBR_EINVAL  a coordinate of V' that is not finite: finite inputs can overflow.  Found ON THE DEVICE with pbr_update_skin's
 *               mechanism — staging buffer, flag word, 4 bytes read back, pointers swapped only then; the normals are written
 *               after that check.
 * OUT OF SCOPE: pbr_multi.h, morphing of anything but positions and normals, topology changes. */
int pbr_set_morph( pbr_ctx* ctx, const uint32_t* vertex_first, const uint32_t* vertex_index, const pbr_float4* vertex_delta,
                   const uint32_t* normal_first, const uint32_t* normal_index, const pbr_float4* normal_delta, uint32_t num_targets );
int pbr_update_morph( pbr_ctx* ctx, const float* weights, uint32_t num_targets );
int pbr_update_pose( pbr_ctx* ctx, const float* weights, uint32_t num_targets, const float* matrices, uint32_t num_bones );
/* DUAL-QUATERNION SKINNING, COMPUTED ON THE DEVICE (ABI version 18).  Linear blending of matrices collapses twisting joints: a ring
 * of vertices blended half and half between a bone and the same bone turned by 180 degrees about the limb's axis ends up ON the
 * axis under pbr_update_skin.  Blending the bones as unit dual quaternions keeps the ring's radius.  This block lifts the item
 * "dual-quaternion skinning" from the OUT OF SCOPE lists above.  pbr_update_skin_dq and pbr_update_pose_dq use the skin that
 * pbr_set_skin set — its influences, its REST POSE, its bone count — and are pbr_update_skin and pbr_update_pose with another
 * blend; they start from the rest pose and never accumulate.  The bones' records lie in the 48 bytes per bone pbr_set_skin
 * allocated (32 are used): the two calls allocate nothing, and pbr_diag_skin_info's byte formula stays true.
 *
 * `dual_quats` is host memory, borrowed for the call, num_bones x 8 floats { rx, ry, rz, rw, dx, dy, dz, dw }: the real part r is
 * the rotation quaternion, vector part first; the dual part is d = 1/2 t r, the quaternion product of ( t, 0 ) and r, t the
 * translation.  A DUAL QUATERNION CARRIES NO SCALE AND NO SHEAR: a bone is a rotation and a translation.
 * THE DEFINITION, operation by operation in binary32, none fused, sqrtf and `/` correctly rounded (the library's default build).
 *   dot4( a, b ) = ( ( ax*bx + ay*by ) + az*bz ) + aw*bw; cross is pbr_denoise_temporal's:
 *   cross( p, q ) = ( py*qz - pz*qy, pz*qx - px*qz, px*qy - py*qx ), each word two products and a subtraction.
 *   1 slots       S = the slots j = 0..3 of the element whose weight compares unequal to 0, in slot order — pbr_update_skin's rule.
 *   2 hemisphere  the pivot is the real part of the first slot of S.  For every later slot s: if dot4( r_s, pivot ) < 0 the
 *                 slot's weight is negated (negation is exact).
 *   3 blend       eight words k: for the first slot Q[k] = w * q_s[k]; for each later slot Q[k] = Q[k] + w * q_s[k] — a
 *                 product, then an addition.
 *   4 normalise   nn = dot4( Q.real, Q.real ), len = sqrtf( nn ), r = Q.real / len, d = Q.dual / len: a division per word, not a
 *                 multiplication by a reciprocal.  Since sqrtf( fl( s*s ) ) == s in binary32, a blend of identity bones comes out
 *                 as the identity for ANY weights.
 *   5 identity    if r.x, r.y, r.z and all four words of d compare equal to 0 and fabsf( r.w ) == 1, the element — position or
 *                 normal — is the rest quad bit for bit; -0 stays -0.
 *   6 position    t = 2.0f * cross( r.xyz, p ); u = cross( r.xyz, t ); p1 = ( p + r.w * t ) + u; c = cross( r.xyz, d.xyz );
 *                 tr = 2.0f * ( ( r.w * d.xyz - d.w * r.xyz ) + c ); p' = p1 + tr; p'.w = p.w bit for bit.
 *   7 normal      the blend comes from the normal's own influences; q = ( n + r.w * t ) + u with t and u of rule 6 taken from n,
 *                 then the tail every normal rule here shares: dd = dot( q, q ); if !( dd > 0 && dd < inf ) n is copied, else
 *                 n'.xyz = q * ( 1.0f / sqrtf( dd ) ), n'.w = n.w.  If !( nn > 0 && nn < inf ) the rest normal is copied too, so no
 *                 normal word is ever NaN.  A position under a blend with nn == 0 or a NaN comes out not finite and is caught by
 *                 rule 8; under an nn that overflowed over finite words (real parts beyond 1.8e19) r and d are 0.
 *   8 overflow    a position that is not finite is found ON THE DEVICE with pbr_update_skin's mechanism — staging buffer, flag
 *                 word, 4 bytes read back, pointers swapped only then; the normals are written after that check.
 * The bones are USED AS GIVEN: not checked for unit length — rule 4 normalises the blend, and a positive multiple of a bone is the
 * same bone up to rounding — and not checked for r . d = 0.  The weights are used as given, as pbr_update_skin uses them.
 * pbr_update_pose_dq is the dual-quaternion skin of the morphed rest pose: rules 1 - 8 on p' and n' of pbr_update_morph's
 * definition, with pbr_update_pose's rules about which normals are morphed and which are skinned.
 * FIVE PROPERTIES that follow, and that tests rest on:
 *   1. UNMOVED ELEMENTS STAY UNMOVED.  Identity bones — ( 0, 0, 0, 1; 0, 0, 0, 0 ) or its negation — under ANY weights give the
 *      rest quads bit for bit; such an element is unmoved for pbr_denoise_temporal.
 *   2. THE SIGN OF A BONE DOES NOT MATTER.  Negating all eight words of any bone changes no bit of V' and N', provided no
 *      element's hemisphere dot is exactly 0.
 *   3. A ONE-HOT ELEMENT FOLLOWS ITS BONE as a rigid motion, whatever the one weight is (a weight that is a power of two gives
 *      the same bits as 1.0f).
 *   4. NOT BIT-EQUAL TO THE MATRIX SKIN.  The results are NOT bit-equal to pbr_update_skin with the equivalent matrices: the
 *      arithmetic differs.
 *   5. pbr_update_pose_dq( 0 weights, Q ) equals pbr_update_skin_dq( Q ) to the bit.
 * THE CONTRACT is pbr_update_skin's: everything behind V' and N' is pbr_update_geometry's.  Boxes, patches, the thick boxes under
 * Phong tessellation, the re-linked ordered walks, renders and the temporal motion path are bit for bit what
 * pbr_update_geometry( V', N' ) and a fresh upload of the moved scene give.  To pbr_diag_skin_info and pbr_diag_morph_info a dq
 * update is another kind (pbr_diag_skin_dq_info, pbr_hip_diag.h, counts them).
 * Refusals, in this order, each leaving the context, the vertices, the normals and the tree exactly as they were:
 *   PBR_EINVAL  a null context;
 *   PBR_ESTATE  pbr_update_skin_dq: no skin set (the message names pbr_set_skin).  pbr_update_pose_dq: pbr_update_pose's
 *               admission — no morph set, no skin set, skin and morph did not capture the same geometry;
 *   PBR_EINVAL  pbr_update_pose_dq: everything pbr_update_morph refuses about `weights` and num_targets;
 *   PBR_EINVAL  about `dual_quats`, in this order: a null pointer; a count other than pbr_set_skin's; a word that is not finite
 *               (the message names bone and word); a real part whose four words are all 0 (the message names the bone);
 *   then pbr_update_geometry's own refusals, in its order;
 *   PBR_EINVAL  rule 8.
 *
 * pbr_dual_quats_from_matrices: host only, no context.  `matrices` are num_bones row-major 3 x 4 matrices in
 * pbr_update_transforms' layout, dual_quats_out has room for num_bones x 8 floats; computed in double and rounded once to float.
 * `message` (may be NULL) receives the reason of a refusal, at most `capacity` bytes with the terminator.  PBR_EINVAL, with
 * nothing written to dual_quats_out, for a null pointer, for a matrix word that is not finite, and for a matrix whose 3 x 3 block R
 * is not a rotation: a word of R^T R - I or det R - 1 above PBR_DQ_RIGID_TOLERANCE in magnitude — a scaled, a sheared and a
 * mirrored matrix are refused, the message names the bone.  The tolerance is an input rule, not a measurement.
 * OUT OF SCOPE: more than four influences, scale or shear on top of the dual quaternions, blending between the linear and the
 * dual-quaternion skin per vertex, pbr_multi.h, topology changes. */
#define PBR_DQ_RIGID_TOLERANCE 1e-4
int pbr_update_skin_dq( pbr_ctx* ctx, const float* dual_quats, uint32_t num_bones );
int pbr_update_pose_dq( pbr_ctx* ctx, const float* weights, uint32_t num_targets, const float* dual_quats, uint32_t num_bones );
int pbr_dual_quats_from_matrices( const float* matrices, uint32_t num_bones, float* dual_quats_out, char* message, size_t capacity );
/* The vertex positions and the vertex normals the context holds now — as uploaded, or after any update of any of the three
 * kinds —, bit for bit, .w included.  pbr_read_bvh's count-only convention: *num_vertices and *num_normals are always set, an
 * output pointer may be NULL, else its capacity (in quads) must reach the count.  *num_normals is 0 for a scene without usable
 * vertex normals (they were not kept).  Before the first geometry update the normals are returned from the host copy the upload
 * keeps.  PBR_EINVAL for a null context, a null count or too little room, PBR_ESTATE without a scene. */
int pbr_read_geometry( pbr_ctx* ctx, pbr_float4* vertices_out, uint32_t vcap, uint32_t* num_vertices,
                       pbr_float4* normals_out, uint32_t ncap, uint32_t* num_normals );
/* The current tree in the wire format: the uploaded nodes, after pbr_update_vertices with the refitted boxes (copied back
 * from the device by this call, not by the update).  *num_nodes = the node count; nodes_out = NULL returns the count only,
 * else capacity >= *num_nodes entries.  A caller's rebuild heuristic (e.g. the growth of the boxes' surface area) reads this. */
int pbr_read_bvh( pbr_ctx* ctx, pbr_bvh_node* nodes_out, uint32_t capacity, uint32_t* num_nodes );

/* CL::loadProgram + createKernel + initKernelArgs (PathTracer.cpp:225-229, :88-125) and
 * initOpenCLBuffers_Textures (:525-533): selects the kernel variant, allocates the three
 * W x H RGBA32F images and zero-fills the input image. */
int pbr_configure( pbr_ctx* ctx, const pbr_config* cfg );

/* CL::updateImageReadOnly( imageIn ) (PathTracer.cpp:61): rgba = W*H*4 floats, row 0 = bottom. */
int pbr_write_input( pbr_ctx* ctx, const float* rgba );
/* Zero the input image and the counters (PathTracer::resetSampleCount + the zero-filled
 * mTextureOut of initOpenCLBuffers_Textures). */
int pbr_reset_accum( pbr_ctx* ctx );

/* clPathTracing (PathTracer.cpp:43-52): set args 0 (seed), 1 (pixelWeight), 2 (pxDim),
 * 3 (camera); CL::execute; CL::finish.  Reads imageIn, writes imageOut and imageDebug. */
int pbr_render_frame( pbr_ctx* ctx, float seed, float pixelWeight, float pxDim, const pbr_camera* cam );

/* Replaces the reference's readImageOutput -> host -> updateImageReadOnly round trip
 * (PathTracer.cpp:61,66): imageOut becomes the next frame's imageIn, on the device. */
int pbr_accumulate( pbr_ctx* ctx );

/* n_frames x { pbr_render_frame( seeds[k], n/(n+1) with n = first_sample_count + k ) ;
 * pbr_accumulate } as one launch over all (pixel, frame) units + one launch that folds the frames into the
 * running mean in frame order — bit-identical to the
 * frame-by-frame sequence.  Needs cam->focusPoint < 0 (depth of field reads another pixel's
 * previous-frame value, pathtracing.cl:58-65): returns PBR_EINVAL otherwise.  The result is
 * left in imageOut AND imageIn (ready to continue). */
int pbr_render( pbr_ctx* ctx, uint32_t first_sample_count, uint32_t n_frames, const float* seeds, float pxDim, const pbr_camera* cam );

/* pbr_render for a camera WITH a focus point (cam->focusPoint >= 0; without one it is pbr_render): bit-identical to
 * n_frames x { pbr_render_frame ; pbr_accumulate } with pixelWeight = n/(n+1), .w included, result in imageOut AND imageIn.
 * What frame k reads of frame k - 1 — the first-hit distance of its own pixel and of the focus pixel — is a chain of
 * camera-ray first hits per pixel; a pre-pass (the focus chain, csrc/pt_chain.hpp) walks it for every local pixel and every
 * frame of a launch, and the frames then go through pbr_render's launch: same tuner, plans, dealing orders and chunking.
 * The pre-pass is not counted (pbr_get_counters, the debug image); pbr_last_kernel_ms includes it.
 * With tile sharding the focus pixel's distance is handed over ONCE PER CALL (pbr_get_focus_depth / pbr_set_focus_depth
 * below; PBR_EINVAL without it): every rank walks the focus pixel's chain itself from there.
 * Phong tessellation (phong_tessellation > 0) with a focus point is refused with PBR_EINVAL: render it with
 * pbr_render_frame + pbr_accumulate per frame. */
int pbr_render_dof( pbr_ctx* ctx, uint32_t first_sample_count, uint32_t n_frames, const float* seeds, float pxDim, const pbr_camera* cam );

/* Adaptive sampling: pbr_render that stops rendering the 8x8 tiles whose mean has converged (not in the reference, which
 * spends the same frames on every pixel).  The call runs in rounds: round 0 renders frames 0 .. min_frames - 1 of every local
 * tile, every later round the next min( round_frames, max_frames - done ) frames of the tiles that are still active; after
 * every round each active tile's error estimate is tested, and a tile that stops never becomes active again.  The k-th frame
 * a pixel renders in this call uses seeds[k] and the weight n/(n+1), n = first_sample_count + k — so a tile that stopped after
 * c frames holds, .w included, bit for bit what pbr_render( first_sample_count, c, seeds ) leaves there; its part of the debug
 * image holds the counts of the last frame it rendered, and pbr_get_counters counts exactly what was traced.  Result in
 * imageOut AND imageIn.
 * The error estimate of a tile with c frames (csrc/pt_adaptive.hpp states it operation by operation, in binary32; it is
 * reproducible to the bit): the relative standard error of the tile's mean luminance,
 *     sqrt( mean over the 64 pixels of var( Y ) / c ) / ( mean over the 64 pixels of mean( Y ) + 0.01 ),
 * Y = 0.2126 r + 0.7152 g + 0.0722 b of a frame's colour, var the sample variance over the c frames of this call.  A tile
 * stops when it is <= threshold; a tile with a frame that is not finite (estimate NaN) stays active.
 * PBR_EINVAL, the context unchanged: a camera with a focus point (every pixel reads the focus pixel's previous frame, and that
 * pixel's tile may stop: pbr_render_dof is the call for depth of field), min_frames < 2, max_frames < min_frames,
 * round_frames = 0, a negative or NaN threshold, null arguments.  Tile sharding and Phong tessellation work as in pbr_render;
 * a rank decides on its own tiles, there is no collective.
 * Schedule: the pinned plan (pbr_diag_pin_plan), else the plan the schedule tuner has kept, else "phased-mid".  An adaptive
 * call does not tune: a caller who wants the tuned plan renders once with pbr_render first.  It leaves the tuner, the learnt
 * tile costs and the dealing orders as they were.
 * AFTER the call the accumulated image has a sample count PER TILE (pbr_read_tile_stats).  Continuing it with a uniform
 * first_sample_count — pbr_render, pbr_render_frame with a weight n/(n+1), another pbr_render_adaptive — is the caller's
 * error: start the next accumulation with pbr_reset_accum / first_sample_count 0. */
typedef struct pbr_adaptive_params {
	uint32_t min_frames;     /* every tile renders at least this many frames; the first test comes after them (>= 2) */
	uint32_t round_frames;   /* frames per further round, a test after every round (>= 1).  A round costs 0.4 - 0.6 ms at 1080p
	                          * (the end of one more launch, the fold, the host's table building: DESIGN.md 5.1i), about what
	                          * one frame costs — 16 frames per round are +4 ... +6 % when nothing stops, 32 half of that */
	uint32_t max_frames;     /* no tile renders more (>= min_frames); seeds[] has max_frames entries */
	float threshold;         /* a tile stops when its error estimate is <= threshold.  0: only tiles whose frames are all the
	                          * same colour stop; +inf: all stop after min_frames */
} pbr_adaptive_params;
int pbr_render_adaptive( pbr_ctx* ctx, uint32_t first_sample_count, const float* seeds, float pxDim, const pbr_camera* cam, const pbr_adaptive_params* params );
/* Of the last pbr_render_adaptive, per LOCAL tile in local-tile order (local tile j = the tile at dealing position
 * j * tile_world + tile_rank, see pbr_config): the frames it rendered, and its error estimate at its last test.  *count =
 * the number of local tiles; frames / error may be NULL (both NULL: *count only), else capacity >= *count entries each.
 * PBR_ESTATE before the first adaptive call after pbr_configure. */
int pbr_read_tile_stats( pbr_ctx* ctx, uint32_t* frames, float* error, uint32_t capacity, uint32_t* count );

/* CL::readImageOutput( imageOut ) / ( imageDebug ) (PathTracer.cpp:66-67).  With tile sharding
 * only this rank's tiles are meaningful (others read 0). */
int pbr_read_output( pbr_ctx* ctx, float* rgba );
int pbr_read_debug( pbr_ctx* ctx, float* rgba );

/* The denoise half of the display step.  The reference's noise filter was never finished
 * (source/opencl/noise_filtering.cl:386-401,417 are TODOs; PathTracer.cpp:155-160 never launches it), so there is no
 * behaviour to match: this keeps its shape — per-pixel first-hit feature buffers (position, normal, texture colour;
 * :441-455), several passes, feature distances over standard deviations (:6-7) — and fills the TODOs with the
 * edge-avoiding a-trous wavelet filter: pass k weighs 5 x 5 taps 2^k pixels apart by
 *   B3-spline * exp( -( |dc|^2 / (sigma_color / 2^k)^2 + |dn|^2 / sigma_normal^2 + |dx|^2 / (sigma_world * 2^k * pxDim * t)^2
 *                       + |da|^2 / sigma_albedo^2 ) ),
 * c the colour, n the first-hit normal (unit, towards the viewer), x the first-hit position, t the centre pixel's
 * first-hit distance (so sigma_world is in pixel footprints), a the first-hit diffuse colour (Kd); taps across the
 * hit / miss divide are left out; a standard deviation of 0 switches its term off.  Features come from one primary ray
 * through every pixel centre over the uploaded scene (orb lights are not in that pass).
 * Each operation is in binary32, and what is not finite has no say: a tap whose exponent is not below inf — NaN included —
 * is left out, and "off" is the term times 0, so a colour that is not finite (or a squared difference that overflows)
 * removes its tap with sigma_color = 0 as well.  A pixel whose weights do not sum to a value in (0, inf) — its own colour is
 * not finite, or ( sigma_world * 2^k * pxDim * t )^2 underflows to 0 while t > 0 — stays as it is.
 *   rgba      host, width x height x 4 floats, row 0 = bottom like pbr_read_output: filtered colour, .w = the
 *             accumulated first-hit distance, unfiltered.  The accumulation itself is not modified.
 *   features  optional (NULL): host, 3 x width x height x 4 floats — position {x, y, z, t (INFINITY: miss)},
 *             normal {x, y, z, hit ? 1 : 0}, albedo {Kd, material index (-1: miss)}.
 * With tile sharding the gathered frame is filtered: call pbr_import_tiles first.  pbr_last_kernel_ms reports the device
 * time of feature pass + filter. */
typedef struct pbr_denoise_params {
	uint32_t passes;      /* 1 .. 8; 5 passes span 61 pixels */
	float sigma_color;
	float sigma_normal;
	float sigma_world;
	float sigma_albedo;
} pbr_denoise_params;
int pbr_denoise( pbr_ctx* ctx, float pxDim, const pbr_camera* cam, const pbr_denoise_params* params, float* rgba, float* features );

/* The variance pbr_render_adaptive estimates anyway, handed to the filter (csrc/pt_denoise_guided.hpp).
 * THE VARIANCE OF A PIXEL.  The last pbr_render_adaptive( first_sample_count = n0 ) left, per pixel, Welford's second moment
 * M2 of the luminance Y = ( 0.2126 r + 0.7152 g ) + 0.0722 b over the c frames its tile rendered (csrc/pt_adaptive.hpp):
 *     var = M2 / (float) ( c - 1 ) / (float) ( n0 + c )         two binary32 divisions, in that order
 * — for n0 = 0 the `v` of the tile's error estimate, the variance of the pixel's mean; for n0 > 0 the sample variance of this
 * call's frames spread over all n0 + c frames of the running mean.  Reproducible to the bit (tests/guided_denoise_ref.py).
 * pbr_read_variance: `variance` = width x height floats, row 0 = bottom like pbr_read_output.
 * STATE.  Both calls need the accumulated image to be what the last pbr_render_adaptive left: PBR_ESTATE (the message names
 * pbr_render_adaptive) before the first adaptive call, and after anything that writes or swaps imageIn / imageOut since —
 * pbr_render_frame, pbr_accumulate, pbr_render, pbr_render_dof, pbr_write_input, pbr_reset_accum, pbr_import_tiles,
 * pbr_configure, another adaptive call that failed.  pbr_read_tile_stats is not bound by this.  PBR_ESTATE with
 * tile_world > 1: the variance of other ranks' tiles is not gathered.  PBR_EINVAL as pbr_denoise: null arguments, passes
 * outside 1 .. 8, a standard deviation that is negative or not finite.  A refused call changes nothing; neither call modifies
 * the accumulation, the moments or the tile stats.
 * THE FILTER is pbr_denoise's a-trous with a luminance term scaled by the LOCAL standard deviation in place of the colour
 * term, and the variance filtered along with the colour — the spatial part of SVGF (Schied et al. 2017) without the temporal
 * one.  Pass k = 0 .. passes - 1, step s = 2^k, works on colour C_k and variance V_k; C_0 = the accumulated image, V_0 = var.
 * For the pixel p, in this order and each operation in binary32:
 *   1. local variance: g = sum G_i G_j V_k( p + (i, j) ) / sum G_i G_j over |i|, |j| <= 1, G = {0.25, 0.5, 0.25} — taps ONE
 *      pixel apart whatever s is; taps outside the image or whose V is not finite are left out; g = 0 if none is left;
 *      sd = sqrt( g )
 *   2. luminance term of a tap q: e_l = | Y( C_k( q ) ) - Y( C_k( p ) ) | / ( sigma_luminance * sd + 1e-6 );
 *      sigma_luminance = 0: e_l = 0
 *   3. e = e_l, plus for a hit centre the normal, world and albedo terms exactly as pbr_denoise has them, added in that order
 *   4. the 5 x 5 taps, s pixels apart, visited row by row (j outer, i inner); skipped: taps outside the image, across the
 *      hit / miss divide, with !( e < inf ), or with V_k( q ) not finite;  w = ( spline_i * spline_j ) * expf( -e )
 *   5. C_k+1( p ) = sum w C_k( q ) / sum w;   V_k+1( p ) = sum ( w * w ) V_k( q ) / ( sum w * sum w );
 *      if sum w is not in (0, inf), colour and variance stay as they were
 * With sigma_luminance = 0 the colour is bit for bit pbr_denoise's with sigma_color = 0 and the same other parameters — on
 * colours that are finite: e_l = 0 does not look at them, so here a tap that is not finite takes part and spreads, where
 * pbr_denoise's colour term times 0 leaves it out.
 *   rgba          host, width x height x 4 floats: filtered colour, .w = the accumulated first-hit distance as pbr_denoise
 *   variance_out  optional (NULL): host, width x height floats, V after the last pass
 *   features      optional (NULL): as pbr_denoise
 * pbr_last_kernel_ms reports the device time of the untile, variance, feature and filter kernels (pbr_read_variance: of
 * the variance kernel). */
int pbr_read_variance( pbr_ctx* ctx, float* variance );
typedef struct pbr_denoise_guided_params {
	uint32_t passes;          /* 1 .. 8 */
	float sigma_luminance;    /* in standard deviations of the pixel's mean; 0 switches the term off */
	float sigma_normal;       /* these three as pbr_denoise_params */
	float sigma_world;
	float sigma_albedo;
} pbr_denoise_guided_params;
int pbr_denoise_guided( pbr_ctx* ctx, float pxDim, const pbr_camera* cam, const pbr_denoise_guided_params* params,
                        float* rgba, float* variance_out, float* features );

/* The temporal part of the variance-guided denoise (csrc/pt_temporal.hpp): pbr_denoise_guided with a per-pixel HISTORY that
 * survives camera moves.  The context keeps, of the previous successful call, the integrated colour and variance, the
 * first-hit features, the history lengths, the camera and pxDim.  A call re-projects that history through the previous
 * camera, rejects it across disocclusions, blends it with the new render by sample weight and runs the guided filter on the
 * result.  Static geometry only (moving geometry would need per-vertex motion: the history is dropped instead, see STATE).
 * THE DEFINITION, operation by operation in binary32 — reproducible to the bit (tests/temporal_ref.py).  C = the accumulated
 * image, V = pbr_read_variance's variance, P | t, N | hit, A | material = the feature buffers of pbr_denoise under `cam`;
 * primes are the previous successful call's: its integrated buffer I', its three feature buffers, its lengths L', its camera
 * (eye', cu', cv', cw' = its u, v, w) and halfPx' = pxDim' * 0.5f.  dot( a, b ) = ( ax*bx + ay*by ) + az*bz.  For the pixel
 * (px, py) of a w x h image:
 *   1. candidate.  Hit pixel: d = P.xyz - eye'.  Miss pixel: d = cw + inner * halfPx of the CURRENT camera, exactly as the
 *      feature pass builds its ray direction before normalizing it — inner = ( ( ( ( cu - cu * (float) w ) + cu * ( 2.0f * (float) px ) )
 *      + cv ) - cv * (float) h ) + cv * ( 2.0f * (float) py ), per component (the sky is at infinity: translation is ignored).
 *      a = dot( d, cu' ) / dot( cu', cu' ), b likewise with cv', c with cw'.  !( c > 0 ): no candidate.
 *      fx = ( a / ( c * halfPx' ) + (float) ( w - 1 ) ) * 0.5f, fy the same with b and h; a value that is not finite: no candidate.
 *      (This inverts the camera-ray construction for an orthogonal basis, which is what PathTracer::fillCameraBasis and
 *      pbrh_camera_lookat hand out; for any other basis the formula is still what is computed.)
 *   2. taps.  x0 = floorf( fx ), tx = fx - x0, likewise y0, ty.  Taps ( x0 + i, y0 + j ), j outer, i inner, i, j in {0, 1};
 *      bw = ( i ? tx : 1 - tx ) * ( j ? ty : 1 - ty ).  A tap is valid if it is inside the image, bw > 0, N'.w == N.w, I' is finite
 *      in all four words, and — for a hit centre — A'.w == A.w, dot( N', N ) >= normal_cos and
 *      squaredDistance3( P', P ) <= r * r with r = ( sigma_world * pxDim ) * P.w (this last term is skipped when sigma_world == 0).
 *   3. history value.  S = sum of bw over the valid taps in visiting order.  S > 0: Hc = ( sum bw * I'.rgb ) / S,
 *      Hv = ( sum ( bw * bw ) * I'.w ) / ( S * S ), Hl = L' of the valid tap with the largest bw (on ties the first in visiting
 *      order).  Otherwise there is no history.
 *   4. blend.  Without history, with C or V not finite, or with max_history == 1: I = {C, V} copied bit for bit, L = 1.
 *      Otherwise L = min( Hl + 1, max_history ), alpha = 1.0f / (float) L, I.rgb = Hc + alpha * ( C - Hc ),
 *      I.w = ( ( 1 - alpha ) * ( 1 - alpha ) ) * Hv + ( alpha * alpha ) * V.  On the first call after the history was dropped no
 *      pixel has a candidate.  (Steps 1 - 3 do not look at max_history: `history` reports them for max_history == 1 too.)
 *   5. filter.  filter->passes passes of pbr_denoise_guided's filter, unchanged, on colour I.rgb and variance I.w; the last pass
 *      restores .w from the accumulated image as pbr_denoise_guided does.
 *   6. store.  I, the three feature buffers, L, cam and pxDim become the history.  What is fed back is the PRE-FILTER I: the
 *      filter's blur does not compound from call to call.
 *   rgba          host, width x height x 4 floats: filtered colour, .w = the accumulated first-hit distance
 *   variance_out  optional (NULL): host, width x height floats, V after the last pass
 *   integrated    optional (NULL): host, width x height x 4 floats: I, .w = the integrated variance — the filter's input
 *   history       optional (NULL): host, width x height x 4 floats {fx, fy, L, valid}: the candidate (NaN, NaN where there is
 *                 none), the history length after this call, the accepted taps as a bit mask (bit 2 * j + i) — all as floats
 * STATE.  Preconditions as pbr_denoise_guided: unsharded, right behind a successful pbr_render_adaptive (PBR_ESTATE otherwise).
 * A second pbr_denoise_temporal without a new successful pbr_render_adaptive in between is PBR_ESTATE: it would integrate the
 * same render twice.  PBR_EINVAL: null cam, temporal, filter or rgba; max_history outside 1 .. 1024; normal_cos outside
 * [-1, 1] or NaN; sigma_world negative or not finite; the filter's argument checks.  The history is dropped — the next call
 * starts at L = 1 everywhere — by pbr_temporal_reset, pbr_configure, pbr_upload_scene and pbr_update_vertices (the last one unless
 * pbr_temporal_track_motion is on, see MOVING GEOMETRY below); NOT by renders,
 * pbr_reset_accum, pbr_denoise or pbr_denoise_guided: a camera move with a fresh accumulation is the use case.  A refused call
 * changes nothing; a successful one does not modify the accumulation, the moments or the tile stats.
 * The history (two sets of four width x height float4 planes + lengths, swapped by pointer, and the filter's working planes)
 * is allocated by the first call after pbr_configure and freed by pbr_configure / pbr_destroy: no allocation per call.
 * pbr_last_kernel_ms reports the device time of the untile, variance, feature, integrate and filter kernels. */
typedef struct pbr_temporal_params {
	uint32_t max_history;   /* 1 .. 1024: cap of the history length L; 1 = no reuse */
	float normal_cos;       /* a history tap is valid if dot( n_prev, n ) >= normal_cos; -1 .. 1 */
	float sigma_world;      /* ... and if |x_prev - x|^2 <= ( sigma_world * pxDim * t )^2; finite, >= 0; 0 = term off */
} pbr_temporal_params;
int pbr_temporal_reset( pbr_ctx* ctx );
int pbr_denoise_temporal( pbr_ctx* ctx, float pxDim, const pbr_camera* cam,
                          const pbr_temporal_params* temporal, const pbr_denoise_guided_params* filter,
                          float* rgba, float* variance_out, float* integrated, float* history );

/* MOVING GEOMETRY: per-vertex motion for pbr_denoise_temporal.  pbr_temporal_track_motion( ctx, 1 ) makes the history survive
 * pbr_update_vertices: the context then keeps H, the vertex positions the history was made under (those current at the last
 * successful pbr_denoise_temporal), and a call that finds the geometry moved asks of every hit pixel "where was this point of
 * the surface when the history was made?" before it looks the history up.  The flag is per context, 0 after pbr_create, needs
 * no scene and survives pbr_configure and pbr_upload_scene (which still drop the history, as does pbr_temporal_reset).  With
 * the flag off nothing changes: pbr_update_vertices drops the history.
 * H: the first successful pbr_update_vertices after a successful pbr_denoise_temporal copies the vertices as they are on the
 * device into a second buffer (device to device, allocated then: 16 bytes per vertex) before it overwrites them; later updates
 * before the next temporal call leave that copy alone; a successful temporal call makes the current vertices H again (nothing
 * is copied).  Turning the flag off frees the buffer, and drops the history if the geometry has moved since it was made.
 * WHICH PATH.  pbr_denoise_temporal (signature unchanged) runs the definition above — the static path, bit for bit — if
 * tracking is off, if there is no history, or if no pbr_update_vertices succeeded since the history was made.  Otherwise the
 * MOTION PATH: step 0 in front, steps 1 and 2 changed as stated, steps 3 - 6 unchanged; `history` keeps its meaning.  All
 * operations binary32, none fused; dot as above; cross( p, q ) = ( py*qz - pz*qy, pz*qx - px*qz, px*qy - py*qx ), each
 * component two products and one subtraction; sqrtf and / correctly rounded.  V = the current vertices, H as above; f = the
 * first-hit face of the pixel, an index into the uploaded facesV (which is in leaf order); a, b, c = the .xyz of
 * V[facesV[f].x], V[facesV[f].y], V[facesV[f].z] and a', b', c' the same corners from H; P, N, A the current features.
 *   0. motion, per hit pixel.  The face is UNMOVED if a == a', b == b', c == c' in all nine coordinates (compared as floats):
 *      Pprev = P.xyz and nref = N.xyz bit for bit, len = 1, code 1.  Otherwise e1 = b - a, e2 = c - a, w = P.xyz - a;
 *      d11 = dot( e1, e1 ), d12 = dot( e1, e2 ), d22 = dot( e2, e2 ); w1 = dot( w, e1 ), w2 = dot( w, e2 );
 *      den = d11 * d22 - d12 * d12; u = ( d22 * w1 - d12 * w2 ) / den; v = ( d11 * w2 - d12 * w1 ) / den;
 *      e1' = b' - a', e2' = c' - a'; Pprev = ( a' + e1' * u ) + e2' * v (a vector times a scalar: per component).
 *      n = cross( e1, e2 ), n' = cross( e1', e2' ); if dot( N, n ) < 0 then n' = -n'; nref = n', NOT normalised;
 *      len = sqrtf( dot( n', n' ) ).  code 2 if u, v and the three words of Pprev are finite, else 3.
 *      A miss pixel has motion {0, 0, 0, 0} and face -1; a hit pixel motion {Pprev, (float) code} and face f.
 *   1. candidate.  Hit pixel: d = Pprev - eye'; with code 3 there is no candidate.  Miss pixels: unchanged.
 *   2. taps.  For a hit centre the normal test is dot( N', nref ) >= normal_cos * len and the distance test
 *      squaredDistance3( P', Pprev ) <= r * r, with r unchanged: ( sigma_world * pxDim ) * P.w.  On an unmoved face these ARE the
 *      static tests ( normal_cos * 1.0f, Pprev = P ).  The material test, the hit / miss test, the finite-history test, the
 *      bilinear weights and the choice of Hl are unchanged.
 * pbr_read_temporal_motion copies the planes of step 0 as the last successful pbr_denoise_temporal left them:
 *   motion  optional (NULL): host, width x height x 4 floats {Pprev.x, Pprev.y, Pprev.z, code}
 *   face    optional (NULL): host, width x height int32
 * PBR_ESTATE before such a call, after pbr_configure, and if that call ran the static path.  Both calls return PBR_ESTATE on
 * an unusable context and PBR_EINVAL for a null one.  The two float4 planes and the face plane (36 bytes per pixel) are
 * allocated by the first call that takes the motion path and freed with the history; nothing is allocated per call.
 * NOT COVERED: tile-sharded contexts (pbr_denoise_temporal refuses them), changes of topology (pbr_update_vertices takes
 * positions only), Phong tessellation (pbr_update_vertices refuses it, unchanged; ray-ordered traversals are covered once
 * pbr_refit_ordered_walk is on — the motion path reads faces and vertices, never a node record), and lights:
 * a light that moves or changes changes the shading, which no test of step 2 sees — call pbr_temporal_reset. */
int pbr_temporal_track_motion( pbr_ctx* ctx, int on );
int pbr_read_temporal_motion( pbr_ctx* ctx, float* motion, int32_t* face );

/* Opt-in fast BVH build on the device: faces in Morton order, clustered bottom-up by
 * surface area, at most 2 faces per leaf, emitted in the reference's flat format — what BVH::getNodes + the packing
 * loops of PathTracer::initOpenCLBuffers_BVH / _Faces (PathTracer.cpp:238-352) produce: `nodes_out` in depth-first order
 * with miss links, `facesV_out` / `facesN_out` = the input faces re-ordered into leaf order.  NOT the reference's builder
 * (accelstructures/BVH.cpp, replicated on the host in host/bvh_builder.cpp): same format, different tree, so images agree
 * statistically, not bit for bit.  All pointers are host memory; nodes_out needs pbr_bvh_node_capacity( num_faces )
 * entries (2 * num_faces - 1: the count actually used comes back in *num_nodes_out).  Vertices must be finite.
 * The clustering's search radius follows the traversal the context is configured with AT THE TIME OF THE CALL (32 for the
 * reference's walk or an unconfigured context, 3 for a ray-ordered one, which such a tree is best walked in: DESIGN.md
 * section 5.4) — so the protocol is pbr_configure( the traversal the tree will be walked in ) BEFORE pbr_build_bvh;
 * pbr_diag_bvh_build_info (pbr_hip_diag.h) tells which radius a build got, the "ploc_radius" knob sets it outright.
 * pbr_last_kernel_ms then reports the device time of the build. */
uint32_t pbr_bvh_node_capacity( uint32_t num_faces );
int pbr_build_bvh( pbr_ctx* ctx, const pbr_float4* vertices, uint32_t num_vertices, const pbr_uint4* facesV, const pbr_uint4* facesN,
                   uint32_t num_faces, pbr_bvh_node* nodes_out, uint32_t* num_nodes_out, pbr_uint4* facesV_out, pbr_uint4* facesN_out );

/* Depth of field with tile sharding.  Every pixel reads the previous-frame distance (.w) of the focus pixel
 * cam->focusPoint (pathtracing.cl:58-65) — the one cross-pixel dependency of the path — and with tile_world > 1 that
 * pixel's tile lives on one rank only.  Per frame: every rank calls pbr_get_focus_depth( x, y ); the rank with
 * *owned = 1 broadcasts *t (one float: ncclBroadcast / MPI_Bcast); every rank passes it to pbr_set_focus_depth and
 * then calls pbr_render_frame with the same camera.  The value is consumed by that frame.  With tile_world = 1 none of
 * this is needed (the kernel reads the pixel itself).  pbr_render_dof needs the same hand-over once per call, whatever
 * its number of frames; the value is consumed by that call. */
int pbr_get_focus_depth( pbr_ctx* ctx, int x, int y, float* t, int* owned );
int pbr_set_focus_depth( pbr_ctx* ctx, float t );

/* The display step the reference leaves to GL (shader/pathtracing.frag:11-15 writes the linear colour to an
 * 8-bit framebuffer): imageOut as width x height RGBA8, each channel floor( clamp( c, 0, 1 ) * 255 + 0.5 ), NaN -> 0,
 * alpha 255, converted on the device (4 B instead of 16 B per pixel over PCIe).  top_row_first = 0: row 0 is the
 * bottom of the image, as pbr_read_output and GL have it; 1: top row first, as image files want it. */
int pbr_read_display( pbr_ctx* ctx, uint8_t* rgba8, int top_row_first );

/* EXPOSURE, TONE CURVE AND sRGB ON THE DEVICE (ABI version 19).  pbr_read_display above is the reference's pass-through shader:
 * no exposure, no transfer function, everything above 1 burns out.  pbr_display turns an HDR image — the accumulated one, or
 * one the caller hands in, such as a denoise call's result — into RGBA8 with an exposure that is given or found from the
 * image's luminance histogram, a tone curve with a shoulder, and linear or sRGB codes.  pbr_read_display stays exactly as it is;
 * { manual, exposure 1, curve 0, transfer 0 } gives its bytes.
 *
 * THE SOURCE.  rgba == NULL reads the accumulated image (imageOut), as pbr_read_display does.  Otherwise rgba is a host image of
 * width x height x 4 floats, row 0 = bottom — what pbr_read_output, pbr_read_full and the three denoise calls return; it is
 * borrowed for the call and copied to a device staging buffer.  Nothing is allocated per call: the buffers are made by the
 * first pbr_display after pbr_configure (the staging buffer by the first one that hands an image in) and freed with the
 * configuration.  The accumulation, the moments and the temporal history are never modified.
 *
 * THE DEFINITION.  Each operation is in binary32 unless it says double, none is fused, `/` is correctly rounded; fmaxf and fminf
 * return the other operand when one is NaN — a signalling NaN too — and fmaxf( -0, 0 ) is +0 (the library writes them as
 * compare-and-select, so this does not depend on a libm).
 *  1 Luminance.  r' = fminf( fmaxf( r, 0 ), FLT_MAX ), likewise g and b: a NaN becomes 0, an infinity FLT_MAX.
 *    Y = ( 0.2126f*r' + 0.7152f*g' ) + 0.0722f*b' (pbr_read_variance's weights).
 *  2 Bin.  Y == 0 counts in `dark`.  Otherwise bin = clamp( (int) ( bits( Y ) >> 20 ) - 888, 0, 255 ): eight bins per octave
 *    over [2^-16, 2^16), everything below in bin 0, everything above — +inf included — in bin 255, Y = 1.0f in bin 128.  Integer
 *    arithmetic on the bit pattern: the histogram is exact and does not depend on the order of the additions.
 *  3 Target, on the host, in double, from the 256 counts n[b].  N = sum n[b]; lo = (double) low_fraction * N;
 *    hi = N - (double) high_fraction * N; with c_b = sum_{i<b} n[i]: kept_b = max( 0, min( c_b + n_b, hi ) - max( c_b, lo ) );
 *    m = ( sum kept_b * ( ( b + 0.5 ) / 8 - 16 ) ) / sum kept_b, both sums in ascending b; log2_target = m clamped to
 *    [min_log2, max_log2].  If N == 0 the target is the remembered value if there is one, else 0.
 *  4 Adaptation.  With no remembered value, or adapt == 1: log2_used = log2_target.  Otherwise
 *    log2_used = prev + (double) adapt * ( log2_target - prev ).  A successful auto call remembers log2_used; pbr_display_reset
 *    and pbr_configure forget it; manual calls neither read nor write it.
 *    exposure = (float) ( (double) key * exp2( -log2_used ) ).  In manual mode exposure is the parameter, and both log2 values
 *    of `info` are 0.
 *  5 Map, per channel c of r, g, b.  x = fminf( fmaxf( c * exposure, 0 ), 65504.0f ).
 *    curve 0: y = x.   curve 1: y = ( x * ( 1.0f + x / ( white * white ) ) ) / ( 1.0f + x ).
 *    curve 2: y = ( x * ( 2.51f * x + 0.03f ) ) / ( x * ( 2.43f * x + 0.59f ) + 0.14f ).
 *    Then y = fminf( fmaxf( y, 0 ), 1 ).  Every curve maps 0 to 0; curve 1 maps x == white to 1.
 *  6 Encode.  transfer 0: (int) floorf( y * 255.0f + 0.5f ), pbr_read_display's arithmetic.  transfer 1: the code is the number
 *    of k in 1 .. 255 with y >= T[k], where T[k] is the smallest binary32 not below x_k, and x_k is the inverse sRGB OETF of
 *    ( k - 0.5 ) / 255 in double: ( ( c + 0.055 ) / 1.055 )^2.4 above 0.04045, c / 12.92 below.  T is a table of constants
 *    (csrc/pt_display_host.hpp): no pow runs per pixel, the encoding is monotone and exact by construction.  Alpha is 255.
 *    Rows are bottom-first, or top-first, as in pbr_read_display.
 * `info` (may be NULL) receives the exposure the map used, the two log2 values, the histogram, counted = N and dark.  Manual
 * mode launches the histogram kernel only when info is given.
 *
 * SHARDED CONTEXTS (tile_world > 1).  With rgba == NULL and manual exposure the call behaves like pbr_read_display: other
 * ranks' tiles read 0 and encode to 0 (and count as dark in `info`).  With rgba == NULL and auto exposure the call returns
 * PBR_ESTATE — a shard's histogram is not the image's; the message says to pass the gathered image (pbr_read_full) as rgba.
 * A host image is always the whole frame.
 *
 * REFUSALS.  Each leaves the context and the remembered exposure unchanged.
 *   PBR_EINVAL  a null context;
 *   PBR_ESTATE  before pbr_configure;
 *   PBR_EINVAL  null params or a null destination; a mode, curve or transfer out of range; a parameter of the ACTIVE mode outside
 *               the ranges its field states, or not finite (the inactive mode's parameters are not looked at; `white` only for
 *               curve 1); the message names the field;
 *   PBR_ESTATE  the sharded auto case above.
 * pbr_last_kernel_ms reports the device time of the histogram and map kernels (not of the copies, not of the host's wait
 * between them).  OUT OF SCOPE: pbr_multi.h, dithering, a luminance-preserving (not per-channel) curve, using the previous
 * call's histogram to avoid the read-back, colour grading. */
#define PBR_DISPLAY_EXPOSURE_MANUAL 0
#define PBR_DISPLAY_EXPOSURE_AUTO 1
#define PBR_DISPLAY_CURVE_CLAMP 0
#define PBR_DISPLAY_CURVE_REINHARD 1
#define PBR_DISPLAY_CURVE_ACES 2
#define PBR_DISPLAY_TRANSFER_LINEAR 0
#define PBR_DISPLAY_TRANSFER_SRGB 1

typedef struct pbr_display_params {
    uint32_t exposure_mode;   /* 0 manual, 1 auto */
    float    exposure;        /* manual: the multiplier, finite and > 0 */
    float    key;             /* auto: the value the scene's trimmed log-mean luminance is mapped to (0.18 is usual); finite, > 0 */
    float    low_fraction;    /* auto: share of the counted pixels dropped at the dark end, >= 0 */
    float    high_fraction;   /* auto: ... at the bright end, >= 0; low + high < 1 */
    float    min_log2, max_log2; /* auto: the log2 mean is clamped to this range; -16 <= min <= max <= 16 */
    float    adapt;           /* auto: in (0, 1]; 1 = jump to the target, less = move that share of the way per call */
    uint32_t curve;           /* 0 clamp, 1 extended Reinhard, 2 ACES fit */
    float    white;           /* curve 1: the input that maps to 1; finite, > 0 */
    uint32_t transfer;        /* 0 linear, 1 sRGB */
} pbr_display_params;

typedef struct pbr_display_info {
    float    exposure;            /* the multiplier the map used */
    double   log2_target;         /* auto: this image's clamped trimmed mean; manual: 0 */
    double   log2_used;           /* auto: after adaptation */
    uint64_t counted, dark;       /* pixels in the histogram / pixels with Y == 0 */
    uint32_t histogram[256];
} pbr_display_info;

int pbr_display( pbr_ctx* ctx, const pbr_display_params* params, const float* rgba /* NULL: the accumulated image */,
                 uint8_t* rgba8, int top_row_first, pbr_display_info* info /* may be NULL */ );
int pbr_display_reset( pbr_ctx* ctx );   /* forget the adapted exposure */

int pbr_get_counters( pbr_ctx* ctx, pbr_counters* out );
/* CL::getKernelTimes (source/CL.cpp:480-488): device time of the last launch, HIP events. */
double pbr_last_kernel_ms( const pbr_ctx* ctx );

/* ---- multi-GPU tile exchange (device pointers; the caller runs the RCCL all-gather — or lets pbr_multi.h do all of it:
 * N contexts in one process, one host thread each, ncclCommInitAll + one ncclAllGather per render) ---- */

/* Bytes of this rank's compact tile buffer: ceil( tiles / tile_world ) * 1024. */
uint64_t pbr_tile_bytes( const pbr_ctx* ctx );
/* Copy this rank's tiles of imageOut (local tile j = the tile at dealing position j * tile_world + tile_rank,
 * see pbr_config; 64 pixels x RGBA32F each) to d_dst on this context's stream and wait. */
int pbr_export_tiles( pbr_ctx* ctx, void* d_dst );
/* d_all = tile_world consecutive rank buffers (all-gather layout).  Scatters every tile into
 * this context's full-frame buffer; the context's own sharding is unchanged. */
int pbr_import_tiles( pbr_ctx* ctx, const void* d_all );
/* The full frame assembled by the last pbr_import_tiles, row-major W x H RGBA32F. */
int pbr_read_full( pbr_ctx* ctx, float* rgba );

#ifdef __cplusplus
}
#endif
#endif
