// libpbrhip.so — implementation of include/pbr_hip.h: context, scene upload / re-layout,
// configuration, launches, read-back and the multi-GPU tile exchange helpers.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <string>
#include <algorithm>
#include <vector>

#include "pbr_hip.h"
#include "pbr_hip_diag.h"
#include "pt_aux.hpp"
#include "pt_adaptive.hpp"
#include "pt_instances.hpp"
// The schedules that were measured and rejected in rounds 1 - 2 (tile, batched, wavefront, pooled: DESIGN.md 5.1b / 5.1d)
// are no longer part of this source; their kernels are kept for the record under lab/src/.
#include "bvh_build.hpp"
#include "pt_denoise.hpp"
#include "pt_denoise_guided.hpp"
#include "pt_temporal.hpp"
#include "pt_temporal_host.hpp"
#include "pt_denoise_host.hpp"
#include "pt_scene_pack.hpp"
#include "pt_tuner.hpp"
#include "pt_deal.hpp"
#include "pt_adaptive_host.hpp"
#include "pt_refit_host.hpp"
#include "pt_refit.hpp"
#include "pt_patch_refit.hpp"
#include "pt_relink.hpp"
#include "pt_transform.hpp"
#include "pt_skin.hpp"
#include "pt_morph.hpp"
#include "pt_skin_dq.hpp"
#include "pt_update_host.hpp"
#include "pt_device_memory.hpp"
#include "pt_display.hpp"

using ptk::DevParams;
using ptmem::Owned;
using ptmem::Pinned;
using ptmem::allocAll;
using ptmem::want;

typedef void ( *KernelFn )( const ptk::DevParams );

// A plan = kernel + persistent grid + LDS split (launch()).  Built once per scene + configuration and kept in the
// context: six occupancy queries and six function-attribute calls are host time a frame-by-frame caller would pay
// on every frame.
struct Plan {
	KernelFn kernel = nullptr;
	int blocks = 0, blockThreads = 0, numHot = 0, park = 0, shade = 0, parkEighths = 4, refillBatch = 0, drainMode = 1;
	size_t ldsBytes = 0;
	const char* name = "";
	char kernelName[96] = "";   // the kernel's symbol as a profiler prints it (without "void " and the argument list)
};

// Experiment and test knobs (pbr_diag_set_knob, include/pbr_hip_diag.h): per context, -1 = the built-in value.  This
// library reads no environment variable; lab scripts and tests set knobs through the diagnostic entry point.
struct Knobs {
	int ldsSlots = -1;      // cap of the node records staged in LDS per block (0 = none)
	int blocksPerCU = -1;   // run below the resident maximum
	int phPark = -1, phShade = -1;   // lane state machine: lanes that leave a node phase before it ends / that wait before a shade phase
	int parkEighths = -1;   // lock-step walk: share of the lanes (in eighths) that leave a node phase before it ends
	int drainMode = -1;     // lane state machine once lanes are DONE: bit 0 scale phPark, bit 1 scale phShade
	int refillBatch = -1;   // lock-step kernels: lanes that wait with a finished unit before the wave refills them together
	int chunkFrames = -1;   // cap of the frames per launch pair (tests: force several launch pairs)
	int faceNormals = -1;   // 0 = recompute the face normal on every hit instead of reading the stored one
	int bvhBuilder = -1;    // pbr_build_bvh: 1 = round 1's radix tree instead of the clustering builder
	int plocRadius = -1;    // pbr_build_bvh: search radius of the clustering builder
	int tuneLog = -1;       // 1 = the schedule tuner logs its launches to stderr
	int dealOrder = -1;     // the queue's dealing order: 0 always spatial, 1 always cost-ordered (once learnt), -1 by the launch's size
	int chainLayout = -1;   // the focus chain's table (pbr_render_dof): 0 frame-major planes (the built-in choice), 1 a pixel slot's frames side by side
	int displayMerge = -1;  // pbr_display's histogram kernel: merge rounds per wave and group before the LDS adds, 0, 1, 2 or 4 (pt_display.hpp)
};

// One dealing order's table: band b's stretch is [ first[b], first[b + 1] ) of host / dev.
struct DealTable {
	std::vector<unsigned> host;
	unsigned first[PT_BANDS + 1] = {};
	Owned<unsigned> dev;
};

// pbr_denoise_temporal's device planes (pt_temporal.hpp), row-major W x H.  Two sets {integrated colour | variance, position,
// normal, albedo} + the history lengths: set `set` holds the previous successful call's, the other one is written by the next
// call and becomes the history by flipping `set` — nothing is copied.  Behind them the filter's working planes, and the
// planes of the motion path (pbr_temporal_track_motion): first-hit face, {Pprev, code}, {nref, len}.
struct TemporalPlanes {
	Owned<float4> integrated[2], position[2], normal[2], albedo[2];
	Owned<unsigned> length[2];
	Owned<float4> ping, pong;
	Owned<float4> info;           // {fx, fy, L, valid} of a call that asks for it
	Owned<float> variance;
	Owned<float4> motion, reference;
	Owned<int> face;
	int set = 0;

	// The planes that are not there yet — the motion path's only if needMotion.  All or nothing: a call that fails gives back
	// what it got, and leaves the planes of earlier calls (a history) alone.
	int alloc( size_t pixels, bool needMotion ) {
		const bool hadHistory = !variance.empty();   // all or nothing: one stands for all
		int err = hadHistory ? 0 : allocAll( { want( integrated[0], pixels ), want( integrated[1], pixels ), want( position[0], pixels ), want( position[1], pixels ),
		                                       want( normal[0], pixels ), want( normal[1], pixels ), want( albedo[0], pixels ), want( albedo[1], pixels ),
		                                       want( ping, pixels ), want( pong, pixels ), want( info, pixels ), want( length[0], pixels ), want( length[1], pixels ),
		                                       want( variance, pixels ) } );

		if( err == 0 && needMotion && face.empty() ) {
			err = allocAll( { want( motion, pixels ), want( reference, pixels ), want( face, pixels ) } );
		}

		if( err != 0 && !hadHistory ) {
			*this = TemporalPlanes();
		}

		return err;
	}
};

// What every pbr_set_* captures (pbr_set_parts, pbr_set_skin, pbr_set_morph): the REST POSE — a copy of the positions and, when
// the call was given the normals' side too, of the normals as they were when it was made —, the staging buffer V' is written to
// before it becomes dVertices (the two buffers are swapped: nothing caches dVertices, every launch takes it from the context),
// and the flag word of a position that is not finite with its pinned host twin.  Each kind owns one: no call touches another
// kind's.  allocRestPose makes one; like the records below it is given back by assigning an empty one.
struct RestPose {
	Owned<float4> dRest, dRestNormals, dStaged;
	Owned<unsigned> dFlag;
	Owned<unsigned, Pinned> hFlag;
	bool normals = false;       // the normals are moved too
	uint64_t bytes = 0;         // device bytes of the kind: the pose and the kind's own tables (formulas in pbr_hip_diag.h)
	uint32_t updates = 0;       // successful updates of the kind since its pbr_set_*
	double lastMs = 0.0;        // of the last of them: device time of the kernels that write V' and N' alone
	uint64_t generation = 0;    // geometryGeneration when the pose was captured
};

// What pbr_set_parts adds to its rest pose: the part index of every vertex and normal, the part records in device and in pinned
// memory.  pbr_set_parts( 0 parts ), a second pbr_set_parts and pbr_upload_scene assign an empty record.  Like the skin's and the
// morph's it knows nothing of ctx->lastUpdate: dropping a kind does not undo that its update was the last one.
struct PartsState {
	RestPose pose;
	uint32_t count = 0;
	Owned<unsigned> dOfVertex, dOfNormal;
	Owned<float4> dRecords;     // six quads per part
	Owned<ptx::PartRecord, Pinned> hRecords;
};

// What pbr_set_skin adds: one 32-byte influence record per vertex and — with normal influences — per normal, the bone records
// (48 bytes each) in device and in pinned memory.  pbr_update_skin_dq and pbr_update_pose_dq (pt_skin_dq_host.hpp) put their
// dual quaternions into the same two tables, 32 of the 48 bytes per bone; pose.updates and pose.lastMs are the matrix skin's, the
// dual-quaternion updates of both calls are counted here.
struct SkinState {
	RestPose pose;
	uint32_t count = 0;
	Owned<uint4> dOfVertex, dOfNormal;   // two quads per element
	Owned<float4> dBones;       // three quads per bone
	Owned<pbr_float4, Pinned> hBones;
	uint32_t dqUpdates = 0;     // successful pbr_update_skin_dq and pbr_update_pose_dq since pbr_set_skin
	double dqLastMs = 0.0;      // of the last of them: device time of the dq kernels that write V' and N' alone
};

// What pbr_set_morph adds: the element-major runs packMorph made — runFirst[count + 1] and one 16-byte entry per delta, for the
// vertices and, with normal targets, for the normals — and the weight table (num_targets floats) in device and in pinned memory.
struct MorphState {
	RestPose pose;
	uint32_t count = 0;
	Owned<uint32_t> dVertexRun, dNormalRun;
	Owned<ptm::Entry> dVertexEntries, dNormalEntries;
	Owned<float> dWeights;
	Owned<float, Pinned> hWeights;
	uint64_t vertexEntries = 0, normalEntries = 0;
};

// The ray-ordered walk (pbr_config.traversal != 0): the records of the configured layout, packed from a host copy of the flat
// tree, and what pbr_refit_ordered_walk's re-link keeps for them (pt_relink_host.hpp, pt_relink.hpp): while that flag is on,
// pbr_update_vertices under a ray-ordered traversal rebuilds dNodesWalk's records on the device.  dRelink: one allocation with
// the static and the working tables of the layout dNodesWalk holds, made by the first such update; relinkView and the two level
// tables point into it.  The tables are a layout's: they go with its records (freeWalkStreams) — with the scene, with a
// pbr_configure of another traversal and with an update that does not re-link.
struct WalkStreams {
	Owned<float4> dNodesWalk;
	uint32_t walkBuilt = 0;        // the scheme dNodesWalk holds (0: none)
	uint32_t walkHotAvail = 0;     // records at the head of dNodesWalk that are ranked for LDS staging (all orders interleaved)
	int walkFirst[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	Owned<unsigned char> dRelink;
	RelinkView relinkView = {};
	unsigned* dRelinkLevelNodes = nullptr;   // inside dRelink
	unsigned* dRelinkLevelFirst = nullptr;
	std::vector<RelinkRun> relinkRuns;
	uint32_t relinkLevels = 0, relinkContainers = 0;
};

// What lives and dies with the uploaded scene: freeScene assigns an empty one.
struct Scene {
	Owned<float4> dNodes;
	Owned<float4> dTris;
	Owned<float4> dTriPN;          // exact vertices + vertex normals per face (Phong tessellation); null if the normal indices are unusable
	Owned<float4> dMats;
	Owned<float4> dFaceN;          // per-face unit normal + material, prepareFaceNormals
	Owned<float4> dLights;
	uint32_t numHotAvail = 0;      // records at the head of the node stream that are ranked for LDS staging
	int firstRef = 0;              // record of node 1
	SceneTree tree;
	WalkStreams walk;
	uint32_t numNodes = 0, numFaces = 0, numMaterials = 0, numLights = 0;
	uint32_t sceneBrdf = 1;
	// pbr_update_vertices (pt_refit_host.hpp, pt_refit.hpp): kept from the upload — the faces' vertex indices, a buffer for the
	// vertices, node 0's box (it has no record), and the refit's tables: thread slots, per-node words and heights, node ->
	// record, the nodes above the cut by level.  refit keeps the verdict, recordOf and the partition's sizes on the host
	RefitPlan refit;
	Owned<uint4> dFacesV;
	Owned<float4> dVertices;
	Owned<float4> dRootBox;
	Owned<unsigned> dRefitSlots;
	Owned<unsigned> dRefitInfo;
	Owned<unsigned short> dRefitHeights;
	Owned<int> dRefitRecordOf;
	Owned<unsigned> dRefitTop;
	Owned<unsigned> dRefitLevelFirst;
	uint32_t numVertices = 0, refitGroups = 0, refitLevels = 0, refitTopNodes = 0, refitSubtrees = 0;
	uint32_t refitUpdates = 0;     // pbr_update_vertices / pbr_update_geometry calls since the upload: > 0 = the boxes are refitted ones
	bool treeStale = false;        // tree.bvh's boxes are older than the device's (refreshTree)
	// pbr_update_geometry (pt_patch_refit_host.hpp, pt_patch_refit.hpp): the faces' normal indices and the vertex normals, kept
	// on the host by the upload (only when dTriPN is there) and moved to the device by the first such update together with the
	// per-face scratch table of thick boxes — no allocation per call
	std::vector<pbr_uint4> patchFacesN;
	std::vector<pbr_float4> patchNormals;
	Owned<uint4> dPatchFacesN;
	Owned<float4> dPatchNormals;
	Owned<float2> dFaceBoxes;      // 24 bytes per face: lo.xyz, hi.xyz
	uint32_t numNormals = 0;       // the upload's count, usable or not
	uint32_t geometryUpdates = 0;  // successful pbr_update_geometry calls since the upload
	float patchAlpha = 0.0f;       // the last update's boxes are thick ones for this phong_tessellation (pbr_configure's state rule)
	// pbr_set_parts / pbr_update_transforms (pt_transform_host.hpp, pt_transform.hpp), pbr_set_skin / pbr_update_skin
	// (pt_skin_host.hpp, pt_skin.hpp), pbr_set_morph / pbr_update_morph / pbr_update_pose (pt_morph_host.hpp, pt_morph.hpp): three
	// kinds of move, independent of each other, each with a RestPose of its own and next to it the tables only that kind has
	// (above).  All of a kind is allocated by its pbr_set_* and given back by the next one and with the scene.  The tables an
	// update uploads have a pinned host twin, so no copy waits for a staging copy of pageable memory.
	PartsState parts;
	SkinState skin;
	MorphState morph;
	// pbr_temporal_track_motion: H, the vertex positions the history was made under — a copy of dVertices taken by the first
	// pbr_update_vertices after a temporal call, allocated then, given back when tracking is turned off (not part of refitBytes)
	Owned<float4> dHistVertices;

	// device bytes of what the upload keeps for updates (pbr_diag_refit_info): nothing for a tree that cannot be refitted
	uint64_t refitBytes() const {
		return !refit.nested ? 0 : dFacesV.bytes() + dVertices.bytes() + dRootBox.bytes() + dRefitSlots.bytes() + dRefitInfo.bytes() + dRefitHeights.bytes()
		                           + dRefitRecordOf.bytes() + dRefitTop.bytes() + dRefitLevelFirst.bytes();
	}
};

// What lives and dies with the configuration: freeImages assigns an empty one.
struct Images {
	Owned<float4> dImgIn;
	Owned<float4> dImgOut;
	Owned<float4> dImgDbg;
	Owned<float4> dRows;           // W x H row-major staging for read-back / write_input
	Owned<float4> dFull;           // all tiles of the frame, filled by pbr_import_tiles
	// the banded queue's dealing orders (pt_deal.hpp; pt_kernel.hpp, nextSlot): the local tiles as a grid cut into PT_BANDS bands
	// of rows, and per order (DealOrder) a table that names, per band, its tiles in the order they are dealt.  deal[kDealSpatial]
	// is the spatial table, or a pinned one; the two cost orders are learnt from the debug image (node visits per pixel of a
	// launch's last frame, learnTileCosts) and keep the spatial bands
	DealTable deal[kDealOrders];
	Owned<float> dTileCost;        // node visits per local tile
	Owned<float4> dFrameBuf;       // frame-parallel launches: {finalColor, focus} per frame and local pixel slot
	// pbr_render_dof: the focus chain's table (pt_chain.hpp) — per frame of a launch and local pixel slot the previous
	// first-hit distance, behind them the focus pixel's per frame
	Owned<float> dChain;
	// pbr_render_adaptive (launchAdaptive, pt_adaptive.hpp): allocated by the first adaptive call after pbr_configure.  Per local
	// tile the frames it rendered, its error estimate at its last test and whether it is still active; per pixel slot the
	// luminance's {mean, M2}; the dealing table of the round (the active tiles only) — the context's own tables stay as they are
	Owned<unsigned> dTileFrames;
	Owned<float> dTileError;
	Owned<unsigned> dTileActive;
	Owned<float2> dMoments;
	Owned<unsigned> dAdaptiveOrder;
	// pbr_denoise_temporal (pt_temporal.hpp): the history's planes, allocated by the first temporal call after pbr_configure
	TemporalPlanes planes;
	// pbr_display (pt_display.hpp): the histogram's 257 counters with their pinned host twin and the sRGB table, made by the
	// first display call after pbr_configure; the staging buffer of a host image, W x H row-major, by the first call that hands one in
	Owned<unsigned> dDisplayCounts;
	Owned<unsigned, Pinned> hDisplayCounts;
	Owned<float> dDisplayTable;
	Owned<float4> dDisplaySource;
};

// The context's stream and events: declared ahead of every buffer, so that they go after the buffers when the context does.
struct Stream {
	hipStream_t s = nullptr;
	Stream() = default;
	Stream( const Stream& ) = delete;
	Stream& operator=( const Stream& ) = delete;
	~Stream() { if( s != nullptr ) { (void) hipStreamDestroy( s ); } }
	operator hipStream_t() const { return s; }
};

struct Event {
	hipEvent_t e = nullptr;
	Event() = default;
	Event( const Event& ) = delete;
	Event& operator=( const Event& ) = delete;
	~Event() { if( e != nullptr ) { (void) hipEventDestroy( e ); } }
	operator hipEvent_t() const { return e; }
};

struct pbr_ctx {
	int device = -1;
	Knobs knobs;
	Stream stream;
	Event evStart, evStop, evTraceStart, evTraceStop, evChainStart;
	Event evRelinkStart, evRelinkStop;
	// the events of the step that computes V' and N' on the device; shared: one update is one kind of move
	Event evXfStart, evXfStop, evXfNormalsStart, evXfNormalsStop;
	Event evFoldStart, evFoldStop;
	Event evHistogramStart, evHistogramStop;   // pbr_display: the histogram kernel (the map kernel: evStart, evStop)
	std::string error;
	double lastKernelMs = 0.0;
	int numCUs = 0;

	// scene
	bool hasScene = false;
	Scene scene;
	double lastRefitUploadMs = 0.0;
	bool refitOrdered = false;     // pbr_refit_ordered_walk's flag: survives pbr_configure and pbr_upload_scene
	double lastRelinkMs = 0.0;     // of the last pbr_update_vertices: device time of the re-link kernels alone,
	uint32_t lastRelinkLaunches = 0;   // their number,
	bool lastRelinked = false;     // and whether it re-linked at all
	// the most recent successful update since the upload (pt_update_host.hpp): what pbr_configure's state rule and the four
	// pbr_diag_*_info calls report of it is derived from this one value.  freeScene resets it, dropping a kind does not
	UpdateKind lastUpdate = UpdateKind::None;
	// which geometry a rest pose was captured from: bumped by an upload and by every successful update; pbr_set_skin and
	// pbr_set_morph record it in their pose, pbr_update_pose needs both to have captured the same
	uint64_t geometryGeneration = 0;

	// configuration + images
	bool configured = false;
	pbr_config cfg;
	int tilesX = 0, tilesY = 0, numTiles = 0, numLocalTiles = 0;
	Images images;
	DealGrid queueGrid;
	bool orderPinned = false;      // pbr_diag_set_tile_order: the caller's order stays (tests, A/B runs)
	std::vector<float> hTileCost;
	bool costLearnt = false;       // the two cost tables hold orders learnt for costCam
	pbr_camera costCam = {};       // the camera (and pixel size) the costs were measured with
	float costPxDim = 0.0f;
	uint32_t launchesSinceLearn = 0;
	char lastDeal[16] = "spatial"; // the order the last render was dealt in
	int lastBvhRadius = 0;         // pbr_build_bvh: the clustering's search radius of the last build (0: none yet / the radix-tree builder)
	bool focusGiven = false;       // pbr_set_focus_depth: the focus pixel's previous-frame distance for the next frame
	float focusDepth = 0.0f;
	Owned<float> dChainCarry;      // pbr_render_dof: the focus pixel's distance after the last launch
	double lastChainMs = 0.0;      // of the last render: time inside the focus chain's launches
	// schedule auto-tuning (launch(), pt_tuner.hpp): per scene + configuration, the candidates are timed on the first
	// frames that are rendered anyway, then the fastest one is kept
	ScheduleTuner tuner;
	Plan plans[ScheduleTuner::kPlans];              // the tuner's candidates; valid while plansBuilt (reset by pbr_upload_scene / pbr_configure / pbr_diag_set_knob)
	Plan phongPlan;                                 // the Phong-tessellation build of the refill kernel (renders every chunk with Phong tessellation)

	Plan chainPlans[ScheduleTuner::kPlans];         // the same candidates in the chained build of their kernels (pbr_render_dof; pt_flavour.hpp)
	bool plansBuilt = false, phongPlanBuilt = false, chainPlansBuilt = false;
	bool workClean = false;                         // the queue heads are zero (foldFrames leaves them so)
	Owned<float, Pinned> hSeeds;                    // pinned staging for the seeds of a launch
	int pinnedPlan = -1;                            // pbr_diag_pin_plan: >= 0 renders with this plan, no tuning (ranks of a multi-GPU run: all the same)
	char lastPlan[48] = "";        // name of the plan that rendered the largest chunk of the last render
	char lastKernel[96] = "";      // ... and its kernel
	double lastTraceMs = 0.0;      // of the last render: time inside the path-tracing launches only ...
	uint32_t lastTraceLaunches = 0; // ... and how many there were (frame-parallel renders are chunked)
	Owned<float> dSeeds;
	Owned<unsigned long long> dCounters;
	Owned<unsigned int> dWork;
	unsigned int* dGuard = nullptr;                 // mapped pinned memory: by hand, pbr_create / pbr_destroy
	bool adaptiveStats = false;          // dTileFrames / dTileError hold the last adaptive call's
	// pbr_read_variance, pbr_denoise_guided: dMoments / dTileFrames describe the accumulated image as it is now — set by a successful
	// adaptive call, cleared by whatever writes or swaps imageIn / imageOut — and that call's first_sample_count
	bool varianceCurrent = false;
	uint32_t varianceFirstCount = 0;
	uint32_t lastAdaptiveRounds = 0;     // of the last adaptive call: rounds (= convergence tests per tile that reached the end),
	uint64_t lastAdaptiveUnits = 0;      // (pixel, frame) units traced,
	double lastAdaptiveFoldMs = 0.0;     // time inside foldFramesAdaptive
	// is set planes.set a history, has the geometry moved since it was made, which path does a call take: pt_temporal_host.hpp.
	// The history is dropped by pbr_temporal_reset, pbr_configure, pbr_upload_scene and — without motion tracking — pbr_update_vertices
	TemporalPolicy temporal;
	bool temporalFresh = false;          // a pbr_render_adaptive succeeded since the last successful temporal call
	pbr_camera temporalCam = {};         // the history's camera and pixel size
	float temporalPxDim = 0.0f;
	// pbr_display: the adapted exposure a successful auto call left, as a log2; forgotten by pbr_display_reset and pbr_configure
	bool displayAdapted = false;
	double displayLog2 = 0.0;
	double lastHistogramMs = 0.0, lastMapMs = 0.0;   // of the last pbr_display (pbr_diag_display_info)
};

// pt_device_memory.hpp's four primitives over the HIP runtime
namespace ptmem {

int deviceAlloc( void** p, size_t bytes ) { return (int) hipMalloc( p, bytes ); }
void deviceFree( void* p ) { (void) hipFree( p ); }
int pinnedAlloc( void** p, size_t bytes ) { return (int) hipHostMalloc( p, bytes, hipHostMallocDefault ); }
void pinnedFree( void* p ) { (void) hipHostFree( p ); }

}  // namespace ptmem

namespace {

int fail( pbr_ctx* ctx, int code, const char* fmt, ... ) {
	char buf[512];
	va_list ap;
	va_start( ap, fmt );
	vsnprintf( buf, sizeof( buf ), fmt, ap );
	va_end( ap );

	if( ctx != nullptr ) {
		ctx->error = buf;
	}

	return code;
}

#define HIP_TRY( ctx, call ) \
	do { \
		const hipError_t err__ = (hipError_t) ( call ); \
		if( err__ != hipSuccess ) { \
			return fail( ctx, PBR_EDEVICE, "%s: %s", #call, hipGetErrorString( err__ ) ); \
		} \
	} while( 0 )

// a step of this library that failed has set the context's error: pass its code on
#define PBR_TRY( call ) \
	do { \
		const int status__ = ( call ); \
		if( status__ != PBR_OK ) { \
			return status__; \
		} \
	} while( 0 )

// What most calls ask of the context first.
int usable( pbr_ctx* ctx ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}
	if( ctx->stream == nullptr ) {
		return fail( ctx, PBR_ESTATE, "context is not usable" );
	}

	return PBR_OK;
}

void freeWalkStreams( pbr_ctx* ctx ) {
	ctx->scene.walk = WalkStreams();
}

void freeScene( pbr_ctx* ctx ) {
	ctx->scene = Scene();
	ctx->lastUpdate = UpdateKind::None;
	ctx->geometryGeneration++;
	ctx->hasScene = false;
}

// Plans carry the scene's, the configuration's and the knobs' values: they are rebuilt on the next render, and the schedule
// tuner starts over (a new scene, a new configuration, a changed knob).
void replan( pbr_ctx* ctx ) {
	ctx->plansBuilt = false;
	ctx->chainPlansBuilt = false;
	ctx->phongPlanBuilt = false;
	ctx->tuner.reset( ScheduleTuner::scaleOf( (size_t) ctx->numLocalTiles * 64 ) );
}

void freeImages( pbr_ctx* ctx ) {
	ctx->images = Images();
	ctx->adaptiveStats = false;
	ctx->varianceCurrent = false;
	ctx->temporal.configure();
	ctx->temporalFresh = false;
	ctx->displayAdapted = false;
	ctx->costLearnt = false;
	ctx->orderPinned = false;
	ctx->configured = false;
}

// queue heads of the pixel-slot queue, one 128-B line each, PT_SUB per band, + the line of the word of heads seen empty (pt_kernel.hpp, nextSlot)
const size_t kWorkBytes = sizeof( unsigned int ) * ( PT_HEADS + 1 ) * PT_BAND_STRIDE;

// frame-parallel launches: cap of the per-frame result buffer (16 B per local pixel and frame)
const size_t kFrameBufBytes = (size_t) 16 << 30;

// 4 public counters (pbr_counters) + 12 slots for experiment statistics (pbr_diag_raw_counters)
const size_t kCounterSlots = 16;


// ---- the path-tracing kernels: one translation unit per plan and build flavour (pt_instances.hpp, pt_instance.hip) ----
// A flavour is a build mode of the same kernel sources (pt_flavour.hpp): bit 0 the ray-ordered walk, bit 1 native
// arithmetic, bit 2 the compact record of the eight-order walk.  A unit that was not linked in (PBR_GUARD builds and the compact
// flavours have no two-paths-per-lane kernels) leaves its picker null.
#define PTI_DECLARE( f, g ) extern "C" const void* PTI_NAME( f, g )( uint32_t, int, int ) __attribute__( ( weak ) );
#define PTI_DECLARE_FLAVOUR( f ) \
	PTI_DECLARE( f, 0 ) PTI_DECLARE( f, 1 ) PTI_DECLARE( f, 2 ) PTI_DECLARE( f, 3 ) PTI_DECLARE( f, 4 ) PTI_DECLARE( f, 5 ) PTI_DECLARE( f, 6 ) PTI_DECLARE( f, 7 ) \
	PTI_DECLARE( f, 8 ) PTI_DECLARE( f, 9 )
PTI_DECLARE_FLAVOUR( 0 )
PTI_DECLARE_FLAVOUR( 1 )
PTI_DECLARE_FLAVOUR( 2 )
PTI_DECLARE_FLAVOUR( 3 )
PTI_DECLARE_FLAVOUR( 5 )     // the compact record of the eight-order walk (flavour bit 2; only together with bit 0)
PTI_DECLARE_FLAVOUR( 7 )
PTI_DECLARE_FLAVOUR( 8 )     // the chained builds (flavour bit 3, pbr_render_dof): groups 3, 8 and 9 stay null
PTI_DECLARE_FLAVOUR( 9 )
PTI_DECLARE_FLAVOUR( 10 )
PTI_DECLARE_FLAVOUR( 11 )
PTI_DECLARE_FLAVOUR( 13 )
PTI_DECLARE_FLAVOUR( 15 )
#define PTI_ROW( f ) { PTI_NAME( f, 0 ), PTI_NAME( f, 1 ), PTI_NAME( f, 2 ), PTI_NAME( f, 3 ), PTI_NAME( f, 4 ), PTI_NAME( f, 5 ), PTI_NAME( f, 6 ), PTI_NAME( f, 7 ), PTI_NAME( f, 8 ), PTI_NAME( f, 9 ) }
#define PTI_NO_ROW { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr }
const pti_picker kPickers[PTI_FLAVOURS][PTI_GROUPS] = { PTI_ROW( 0 ), PTI_ROW( 1 ), PTI_ROW( 2 ), PTI_ROW( 3 ), PTI_NO_ROW, PTI_ROW( 5 ), PTI_NO_ROW, PTI_ROW( 7 ),
                                                       PTI_ROW( 8 ), PTI_ROW( 9 ), PTI_ROW( 10 ), PTI_ROW( 11 ), PTI_NO_ROW, PTI_ROW( 13 ), PTI_NO_ROW, PTI_ROW( 15 ) };

KernelFn pickKernel( int flavour, int group, uint32_t brdf, bool shadow, bool lights ) {
	const pti_picker pick = kPickers[flavour][group];
	return ( pick != nullptr ) ? (KernelFn) pick( brdf, shadow ? 1 : 0, lights ? 1 : 0 ) : nullptr;
}

// the flavour a configuration renders with
int flavourOf( uint32_t traversal, uint32_t arith ) {
	return ( ( traversal != 0 ) ? 1 : 0 ) | ( ( arith != 0 ) ? 2 : 0 ) | ( ( traversal == PBR_WALK_EIGHT_ORDERS_COMPACT ) ? 4 : 0 );
}

int flavourOf( const pbr_config& cfg ) {
	return flavourOf( cfg.traversal, cfg.arith );
}

// The two-paths-per-lane kernel (pt_dual.hpp) exists where its hand-scheduled two-walk node phase does: not in builds
// without the assembly node phases, not over compact records — those render plan 6 with the 6-waves state machine.
bool dualIsDual( int flavour );

// the "mid" budget: <= 80 VGPRs, launched as two 768-thread blocks per CU = 6 waves / SIMD
const int kMidBlockThreads = 768;

// two paths per lane (pt_dual.hpp).  Its node phase is hand-scheduled only: builds without PT_NODE_PHASE_ASM (PBR_GUARD,
// PBR_NODE_PHASE_CXX) render the plan with the 6-waves state machine — same bits, every loop bounded.
const bool kDualIsDual =
#ifdef PT_NODE_PHASE_ASM
	true;
#else
	false;
#endif

bool dualIsDual( int flavour ) {
	return kDualIsDual && ( flavour & 4 ) == 0;
}

// Scenes whose tree does not fit the staged LDS prefix ("large": the walk is most of a bounce) and those whose tree
// does ("small": shading is): the lock-step walk's park share and refill batch differ between the two.
const uint32_t kWideMinNodes = 2048;

// lock-step kernels: lanes of a wave that wait with a finished unit before they take their next units together.  Measured
// (profiles/r03/experiments/sweep_refill.txt, 1080p): Cornell refill-mid 4791 / 4837 / 4865 / 4765 / 4570 Msamples/s at
// 1 / 8 / 16 / 24 / 32 lanes (a single frame: 2197 -> 2437), Sponza-class refill-wide 1618 / 1664 / 1751 / 1776 / 1791:
// 16 where the tree fits LDS and shading is most of a bounce, 32 where the walk is.
const int kRefillBatchSmall = 16, kRefillBatchLarge = 32;

// PHONGTESS == 1: the lock-step kernel in the LEAN budget (round 4).  The long cubic solve spills in every budget — 336 B /
// 272 B / 72 B of scratch per lane at 64 / 80 / 128 registers — and 4 waves with 8 spilled registers beat 8 waves with 208:
// 4133 against 2731 Msamples/s on a 288-face sphere over a floor at 1080p, 2850 against 2015 on a 9 000-face one
// (profiles/r04/experiments/phong_register_budget.txt; rounds 2-3 built it in the 64-register budget).


// {magic, shifts} with which ptk::divInvariant divides any 32-bit n by d exactly (d = 0 is never divided by: as 1)
void invariantDivisor( unsigned d, unsigned out[2] ) {
	d = ( d == 0u ) ? 1u : d;
	unsigned l = 0;

	while( ( 1ull << l ) < (unsigned long long) d ) {
		l++;
	}

	const unsigned long long magic = ( ( 1ull << 32 ) * ( ( 1ull << l ) - d ) ) / d + 1ull;
	out[0] = (unsigned) magic;
	out[1] = ( l < 1u ? l : 1u ) | ( ( l > 0u ? l - 1u : 0u ) << 8 );
}

// The ray-ordered walk's records of a layout (pt_scene_pack.hpp, packWalk) to the device, in place of the ones there were.
int uploadWalkStreams( pbr_ctx* ctx, const PackedWalk& walk, uint32_t layout ) {
	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	freeWalkStreams( ctx );
	HIP_TRY( ctx, ctx->scene.walk.dNodesWalk.alloc( walk.storage.size() ) );
	HIP_TRY( ctx, hipMemcpy( ctx->scene.walk.dNodesWalk, walk.storage.data(), sizeof( Quad ) * walk.storage.size(), hipMemcpyHostToDevice ) );
	std::memcpy( ctx->scene.walk.walkFirst, walk.first, sizeof( ctx->scene.walk.walkFirst ) );
	ctx->scene.walk.walkHotAvail = walk.hotSlots;
	ctx->scene.walk.walkBuilt = layout;
	return PBR_OK;
}

// The host copy of the tree after pbr_update_vertices: the boxes come back from the device when somebody asks for them
// (pbr_read_bvh, a ray-ordered walk to build) — an update itself copies nothing back.
int refreshTree( pbr_ctx* ctx ) {
	if( !ctx->scene.treeStale ) {
		return PBR_OK;
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	std::vector<Quad> records( ctx->scene.dNodes.count() );
	Quad root[2];
	HIP_TRY( ctx, hipMemcpy( records.data(), ctx->scene.dNodes, ctx->scene.dNodes.bytes(), hipMemcpyDeviceToHost ) );
	HIP_TRY( ctx, hipMemcpy( root, ctx->scene.dRootBox, sizeof( root ), hipMemcpyDeviceToHost ) );
	std::vector<pbr_bvh_node>& bvh = ctx->scene.tree.bvh;
	bvh[0].bbMin = pbr_float4 { root[0].x, root[0].y, root[0].z, bvh[0].bbMin.w };
	bvh[0].bbMax = pbr_float4 { root[1].x, root[1].y, root[1].z, bvh[0].bbMax.w };

	for( uint32_t i = 1; i < ctx->scene.tree.size(); i++ ) {
		const Quad* rec = records.data() + (size_t) ctx->scene.refit.recordOf[i] * 2;
		bvh[i].bbMin = pbr_float4 { rec[0].x, rec[0].y, rec[1].x, bvh[i].bbMin.w };
		bvh[i].bbMax = pbr_float4 { rec[0].z, rec[0].w, rec[1].y, bvh[i].bbMax.w };
	}

	ctx->scene.treeStale = false;
	return PBR_OK;
}

int buildWalkStreams( pbr_ctx* ctx, uint32_t layout ) {
	PBR_TRY( refreshTree( ctx ) );
	PackedWalk walk;
	PBR_TRY( packWalk( ctx->scene.tree, layout, &walk, &ctx->error ) );
	return uploadWalkStreams( ctx, walk, layout );
}

// The node stream, its ranked prefix and the first record(s) for the configured traversal.
int applyWalk( pbr_ctx* ctx, DevParams* P, uint32_t* hotAvail ) {
	const uint32_t scheme = ctx->configured ? ctx->cfg.traversal : 0u;
	P->nodes = ctx->scene.dNodes;
	P->firstRef = ctx->scene.firstRef;
	P->walkScheme = 0;
	*hotAvail = ctx->scene.numHotAvail;

	if( scheme == 0 ) {
		return PBR_OK;
	}

	if( ctx->scene.walk.walkBuilt != scheme ) {
		PBR_TRY( buildWalkStreams( ctx, scheme ) );
	}

	P->nodes = ctx->scene.walk.dNodesWalk + 2;   // behind the 32-byte header ...
	P->walkTable = (const int*) ctx->scene.walk.dNodesWalk.get();   // ... which the kernels read through a pointer of its own (DevParams)
	P->firstRef = ctx->scene.walk.walkFirst[0];
	P->walkScheme = (int) scheme;
	*hotAvail = ctx->scene.walk.walkHotAvail;
	return PBR_OK;
}

// What a mode needs beyond valid numbers, checked where the mode is CHOSEN (pbr_configure, and pbr_upload_scene of a
// configured context) instead of in the middle of a viewer's render loop: the mode's kernels are linked in, and —
// for a tree (null: none to walk) — its records can be built.  They are packed here, before the caller changes the context
// (ADVICE r06): a mode or a scene the walk cannot take (a tree that is not properly nested, too many nodes for 31-bit record
// references) leaves the context as it was.
int packConfiguredWalk( pbr_ctx* ctx, const pbr_config& cfg, const SceneTree* tree, PackedWalk* walk ) {
	if( pbr_mode_built( cfg.traversal, cfg.arith ) != 1 ) {
		return fail( ctx, PBR_ESTATE, "this library was built without the kernels of traversal %u / arith %u (pbr_mode_built)", cfg.traversal, cfg.arith );
	}
	if( tree == nullptr || cfg.traversal == 0 ) {
		return PBR_OK;
	}

	return packWalk( *tree, cfg.traversal, walk, &ctx->error );
}

// ---- the dealing orders of the banded queue: the device side (the orders themselves, and which one a call gets: pt_deal.hpp) ----
int uploadTileOrder( pbr_ctx* ctx ) {
	const DealTable& table = ctx->images.deal[kDealSpatial];
	HIP_TRY( ctx, hipMemcpyAsync( table.dev, table.host.data(), sizeof( unsigned ) * table.host.size(), hipMemcpyHostToDevice, ctx->stream ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );   // the source is pageable: do not let it change under the copy
	return PBR_OK;
}

// After a launch: node visits per local tile from the debug image (the launch's last frame), then the cost order.  Runs when
// there is no order yet or the camera has moved since it was learnt (then at most every 16th launch: an order learnt a few
// frames ago is nearly as good, and the read-back is a synchronisation a frame-by-frame caller should not pay per frame).
int learnTileCosts( pbr_ctx* ctx, const pbr_camera* cam, float pxDim ) {
	if( ctx->orderPinned || ctx->knobs.dealOrder == 0 || ctx->images.deal[kDealCostClasses].dev == nullptr ) {
		return PBR_OK;
	}

	const bool moved = !ctx->costLearnt || std::memcmp( &ctx->costCam, cam, sizeof( pbr_camera ) ) != 0 || ctx->costPxDim != pxDim;

	if( !moved || ( ctx->costLearnt && ctx->launchesSinceLearn < 16u ) ) {
		return PBR_OK;
	}

	const unsigned tiles = (unsigned) ctx->numLocalTiles;
	hipLaunchKernelGGL( ptk::tileCosts, dim3( ( tiles + 3u ) / 4u ), dim3( 256 ), 0, ctx->stream, (const float4*) ctx->images.dImgDbg, ctx->images.dTileCost, tiles );
	HIP_TRY( ctx, hipGetLastError() );
	ctx->hTileCost.resize( tiles );
	HIP_TRY( ctx, hipMemcpyAsync( ctx->hTileCost.data(), ctx->images.dTileCost, sizeof( float ) * tiles, hipMemcpyDeviceToHost, ctx->stream ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	std::vector<unsigned> spatial;
	DealTable& classes = ctx->images.deal[kDealCostClasses];
	DealTable& last = ctx->images.deal[kDealExpensiveLast];
	spatialTileOrder( ctx->queueGrid, ctx->numLocalTiles, PT_BANDS, &spatial, classes.first );
	std::copy( classes.first, classes.first + PT_BANDS + 1, last.first );
	costTileOrder( classes.first, PT_BANDS, spatial, ctx->hTileCost, &classes.host );
	expensiveLastTileOrder( last.first, PT_BANDS, spatial, ctx->hTileCost, &last.host );
	HIP_TRY( ctx, hipMemcpyAsync( classes.dev, classes.host.data(), sizeof( unsigned ) * classes.host.size(), hipMemcpyHostToDevice, ctx->stream ) );
	HIP_TRY( ctx, hipMemcpyAsync( last.dev, last.host.data(), sizeof( unsigned ) * last.host.size(), hipMemcpyHostToDevice, ctx->stream ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	ctx->costLearnt = true;
	ctx->costCam = *cam;
	ctx->costPxDim = pxDim;
	ctx->launchesSinceLearn = 0;
	return PBR_OK;
}

// The scene for the path-tracing, diagnostic and denoise kernels, walked in the configured order (pbr_config.traversal);
// hotAvail: the ranked prefix of that stream.  Returns PBR_OK, or why the configured walk's streams could not be built (the
// caller fails with it — no silent walk in another order).
int sceneParams( pbr_ctx* ctx, DevParams* P, uint32_t* hotAvail = nullptr ) {
	std::memset( P, 0, sizeof( *P ) );
	uint32_t hot = 0;
	const int walk = applyWalk( ctx, P, &hot );

	if( hotAvail != nullptr ) {
		*hotAvail = hot;
	}

	P->parkEighths = 4;
	P->tris = ctx->scene.dTris;
	P->faceN = ctx->scene.dFaceN;
	P->mats = ctx->scene.dMats;
	P->lights = ctx->scene.dLights;
	P->guard = ctx->dGuard;
	P->numNodes = (int) ctx->scene.numNodes;
	P->numLights = (int) ctx->scene.numLights;
	return walk;
}

// The camera of a w x h image: its vectors, and the launch-invariant sub-expressions of initRay (pt_kernel.hpp), as
// ptd::cameraTerms computes them (pt_denoise_host.hpp: host arithmetic, built with -ffp-contract=off like the kernels).
ptd::CameraTerms setCamera( DevParams* P, const pbr_camera* cam, int w, int h, float pxDim ) {
	const ptd::CameraTerms C = ptd::cameraTerms( *cam, w, h, pxDim );
	ptd::copy3( P->eye, C.eye );
	ptd::copy3( P->cu, C.cu );
	ptd::copy3( P->cv, C.cv );
	ptd::copy3( P->cw, C.cw );
	ptd::copy3( P->camA, C.camA );
	ptd::copy3( P->cvH, C.cvH );
	P->halfPx = C.halfPx;
	P->pxDim = C.pxDim;
	P->width = w;
	P->height = h;
	return C;
}

// The image kernels (untile, display, features, variance, the filters): one thread per pixel, 64 x 4 blocks.
const dim3 kImageBlock( 64, 4 );

dim3 imageGrid( int w, int h ) {
	return dim3( ( w + 63 ) / 64, ( h + 3 ) / 4 );
}

// The end of a call that recorded evStart and evStop around its kernels: wait for the stream, keep the time between the two.
int timedTail( pbr_ctx* ctx ) {
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	float ms = 0.0f;
	HIP_TRY( ctx, hipEventElapsedTime( &ms, ctx->evStart, ctx->evStop ) );
	ctx->lastKernelMs = (double) ms;
	return PBR_OK;
}

// A plan's recipe: kernel group, name, the state machine's thresholds, block size, and the per-lane path state that two
// paths per lane keep in LDS behind the staged prefix.
struct PlanSpec {
	int group;
	const char* name;
	int park, shade;
	int blockThreads = PBR_BLOCK;
	size_t pathSlotBytes = 0;
};

// A plan = kernel + persistent grid + LDS split.  Grid: as many blocks as stay resident, never more
// than there is work for.  LDS: each block stages a prefix of the node stream; the CU's 160 KB are
// split between the blocks the register budget admits.  The experiment knobs (PBR_BLOCKS_PER_CU, PBR_LDS_SLOTS,
// PBR_PH_PARK, PBR_PH_SHADE, PBR_PARK_EIGHTHS, PBR_DRAIN_MODE, PBR_REFILL_BATCH) are read when the plans are built — once per
// scene + configuration — not per launch.
int makePlan( pbr_ctx* ctx, const PlanSpec& spec, uint32_t hotAvail, Plan* plan, bool chained = false ) {
	const Knobs& knobs = ctx->knobs;
	const int flavour = flavourOf( ctx->cfg ) | ( chained ? PTI_CHAINED : 0 );
	const bool lights = ( ctx->scene.numLights > 0 );
	const bool shadow = ( ctx->cfg.shadow_rays == 1 ) && lights;
	const KernelFn kernel = pickKernel( flavour, spec.group, ctx->cfg.brdf, shadow, lights );

	if( kernel == nullptr ) {
		return fail( ctx, PBR_ESTATE, "plan %s: this library was built without that kernel (flavour %d)", spec.name, flavour );
	}

	int blocksPerCU = 0;
	HIP_TRY( ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor( &blocksPerCU, (const void*) kernel, spec.blockThreads, 0 ) );
	blocksPerCU = ( blocksPerCU < 1 ) ? 1 : blocksPerCU;

	if( knobs.blocksPerCU >= 1 && knobs.blocksPerCU < blocksPerCU ) {
		blocksPerCU = knobs.blocksPerCU;
	}

	// a block's share of the CU's 160 KB, for the staged tree top
	const size_t ldsPerCU = 160 * 1024;
	const size_t share = ldsPerCU / (size_t) blocksPerCU - 256;
	const size_t slotBytes = spec.pathSlotBytes;     // two paths per lane: 2 slots x 4 planes x 16 B of path state per lane behind the staged prefix

	// (a toolchain that fitted such a kernel into fewer registers would report two blocks per CU, whose share
	// is smaller than the path slots — the subtraction below is unsigned)
	if( share < slotBytes + 32 ) {
		return fail( ctx, PBR_ESTATE, "plan %s: %zu B of per-lane path state do not fit a block's %zu B share of LDS at %d blocks per CU", spec.name, slotBytes, share, blocksPerCU );
	}

	size_t slots = ( share - slotBytes ) / 32;
	slots = std::min<size_t>( slots, hotAvail );

	if( knobs.ldsSlots >= 0 ) {
		slots = std::min<size_t>( slots, (size_t) knobs.ldsSlots );
	}
	if( flavour & 4 ) {
		slots &= ~(size_t) 1;      // compact records are two slots each: a staged prefix ends on a record
	}

	// the limit is a property of the kernel function, shared by every context of the process: always the block's whole
	// share, so that a context with a small scene never lowers it under another context's cached plan
	HIP_TRY( ctx, hipFuncSetAttribute( (const void*) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) share ) );

	plan->kernel = kernel;
	plan->blockThreads = spec.blockThreads;
	plan->blocks = ctx->numCUs * blocksPerCU;   // all that are resident at once; runPlan() launches fewer when there is less work
	plan->numHot = (int) slots;
	plan->ldsBytes = slots * 32 + slotBytes;
	plan->park = spec.park;
	plan->shade = spec.shade;
	plan->parkEighths = ( ctx->scene.numNodes >= kWideMinNodes ) ? 4 : 6;   // see traverse(), pt_kernel.hpp
	plan->refillBatch = ( knobs.refillBatch >= 1 ) ? std::min( 64, knobs.refillBatch ) : ( ( ctx->scene.numNodes >= kWideMinNodes ) ? kRefillBatchLarge : kRefillBatchSmall );
	// pathTracingPhased once lanes are DONE, 1: measured (single-frame 1080p launches): park share scaled, shade threshold as is:
	// Dragon-class 2.99 -> 2.47 ms, hairball 4.26 -> 4.02 ms, Sponza- / Cornell-class unchanged; scaling the shade threshold too
	// helps the first two further (2.26 / 3.56 ms) and costs the others 10 - 20 %
	plan->drainMode = ( knobs.drainMode >= 0 ) ? knobs.drainMode : 1;

	if( knobs.phPark >= 0 ) {
		plan->park = std::max( 1, std::min( ( spec.pathSlotBytes != 0 ) ? 128 : 64, knobs.phPark ) );   // two paths per lane: walks of up to 128 per wave
	}
	if( knobs.phShade >= 0 ) {
		plan->shade = std::max( 1, std::min( 64, knobs.phShade ) );
	}
	if( knobs.parkEighths >= 0 ) {
		plan->parkEighths = std::min( 8, knobs.parkEighths );
	}

	plan->name = spec.name;
	// the symbol as rocprofv3 prints it (pt_instance.hip instantiates exactly these; namespaces: pt_flavour.hpp)
	const char* const tf[2] = { "false", "true" };
	const int minw[PTI_GROUPS] = { 4, 6, 8, 4, 4, 6, 8, 0, 0, 0 };

	if( spec.group == PTI_DUAL ) {
		std::snprintf( plan->kernelName, sizeof( plan->kernelName ), "ptk_f%d::pathTracingDual<%u, %s, %s>", flavour, ctx->cfg.brdf, tf[shadow], tf[lights] );
	}
	else if( spec.group >= PTI_PHASED_LEAN ) {
		std::snprintf( plan->kernelName, sizeof( plan->kernelName ), "ptk_f%d::pathTracingPhased<%u, %s, %s, %d>", flavour, ctx->cfg.brdf, tf[shadow], tf[lights], minw[spec.group] );
	}
	else {
		std::snprintf( plan->kernelName, sizeof( plan->kernelName ), "ptk_f%d::pathTracing<%u, %s, %s, %d, %s>", flavour, ctx->cfg.brdf, tf[shadow], tf[lights], minw[spec.group], tf[spec.group == PTI_REFILL_PHONG] );
	}

	return PBR_OK;
}

// The plans of this scene + configuration, built on the first render after replan(): the tuner's candidates, and with Phong
// tessellation the one plan that renders it.
int buildPlans( pbr_ctx* ctx, uint32_t hotAvail, bool phong, bool chained ) {
	if( !ctx->plansBuilt || ( chained && !ctx->chainPlansBuilt ) ) {
		const int flavour = flavourOf( ctx->cfg );
		// The state machine's thresholds (lanes that leave a node phase before it ends / lanes that wait before a shade phase):
		// 16 / 40 in the reference's walk (profiles/r03/experiments/sweep_thresholds.txt).  A ray-ordered walk makes fewer visits per
		// shading, and its 6-waves build does best at 12 / 48: Dragon-class +1.5 % (exact) / +2.5 % (native), hairball +0.1 … +0.3 %,
		// Sponza-class -0.3 … -1.2 % — where the two-paths plan wins anyway (profiles/r05/experiments/sweep_thresholds_ordered_walk*.txt).
		const bool orderedWalk = ( flavour & 1 ) != 0;
		const PlanSpec specs[ScheduleTuner::kPlans] = {
			{ PTI_REFILL_LEAN, "refill-lean", 0, 0 },
			{ PTI_REFILL_WIDE, "refill-wide", 0, 0 },
			{ PTI_PHASED_LEAN, "phased-lean", 16, 32 },
			{ PTI_PHASED_WIDE, "phased-wide", 16, 48 },
			{ PTI_PHASED_MID, "phased-mid", orderedWalk ? 12 : 16, orderedWalk ? 48 : 40, kMidBlockThreads },
			{ PTI_REFILL_MID, "refill-mid", 0, 0, kMidBlockThreads },
			// 28 of a wave's up to 128 walks leave a node phase before it ends; a shade phase waits for 48 lanes (measured:
			// profiles/r04/experiments/two_paths_per_lane.txt).  Without the hand-scheduled node phase: phased-mid's kernel and thresholds.
			dualIsDual( flavour ) ? PlanSpec{ PTI_DUAL, "phased-dual", 28, 48, PBR_BLOCK, (size_t) 2 * 4 * 16 * PBR_BLOCK }
			                      : PlanSpec{ PTI_PHASED_MID, "phased-dual", 16, 40, kMidBlockThreads },
		};

		for( int k = 0; k < ScheduleTuner::kPlans; k++ ) {
			if( !ctx->plansBuilt ) {
				PBR_TRY( makePlan( ctx, specs[k], hotAvail, &ctx->plans[k] ) );
				ctx->tuner.names[k] = specs[k].name;
			}
			if( chained && !ctx->chainPlansBuilt ) {
				PBR_TRY( makePlan( ctx, specs[k], hotAvail, &ctx->chainPlans[k], true ) );
			}
		}

		ctx->chainPlansBuilt = ctx->chainPlansBuilt || chained;

		ctx->tuner.log = ( ctx->knobs.tuneLog > 0 ) ? stderr : nullptr;
		ctx->phongPlanBuilt = ctx->plansBuilt && ctx->phongPlanBuilt;
		ctx->plansBuilt = true;
	}

	if( phong && !ctx->phongPlanBuilt ) {
		// the Phong-tessellation build of the lock-step kernel (lean budget)
		PBR_TRY( makePlan( ctx, PlanSpec{ PTI_REFILL_PHONG, "refill-lean-phong", 0, 0 }, hotAvail, &ctx->phongPlan ) );
		ctx->phongPlanBuilt = true;
	}

	return PBR_OK;
}

// waveUnits: how many wave-sized pieces of work the launch has — tiles x frames (a rank of an 8-GPU run has 4050
// tiles at 1080p: fewer than the 6144 - 8192 resident waves, but 256 frames of them)
int runPlan( pbr_ctx* ctx, const Plan& plan, DevParams* P, size_t waveUnits ) {
	const size_t wavesPerBlock = (size_t) plan.blockThreads / 64;
	const size_t needed = std::max<size_t>( 1, ( waveUnits + wavesPerBlock - 1 ) / wavesPerBlock );
	const unsigned blocks = (unsigned) std::min<size_t>( (size_t) plan.blocks, needed );
	P->numHot = plan.numHot;
	P->numHotBytes = plan.numHot * 32;
	P->slotBase = plan.numHot * 32;
	P->phPark = plan.park;
	P->phShade = plan.shade;
	P->refillBatch = plan.refillBatch;
	P->drainMode = plan.drainMode;
	P->parkEighths = plan.parkEighths;
	hipLaunchKernelGGL( plan.kernel, dim3( blocks ), dim3( (unsigned) plan.blockThreads ), plan.ldsBytes, ctx->stream, *P );
	HIP_TRY( ctx, hipGetLastError() );
	return PBR_OK;
}

// The caller's seeds go to the device through a pinned staging buffer: a copy from pageable memory is staged synchronously
// by the runtime.
int stageSeeds( pbr_ctx* ctx, const float* seeds, uint32_t nFrames ) {
	HIP_TRY( ctx, ctx->dSeeds.grow( nFrames ) );
	HIP_TRY( ctx, ctx->hSeeds.grow( std::max<size_t>( nFrames, 64 ) ) );
	std::memcpy( ctx->hSeeds, seeds, sizeof( float ) * nFrames );
	HIP_TRY( ctx, hipMemcpyAsync( ctx->dSeeds, ctx->hSeeds, sizeof( float ) * nFrames, hipMemcpyHostToDevice, ctx->stream ) );
	return PBR_OK;
}

// Frame-parallel schedules: every (pixel, frame) is its own unit of work — the frames of a pixel are
// independent up to the running mean (pathtracing.cl:28,255,332) — so a launch ends with single
// frames in flight, not with whole pixels; {finalColor, focus} of each go to dFrameBuf and
// foldFrames applies setColors in frame order.  The buffer (16 B per pixel and frame) is capped,
// longer renders run as several launch pairs.  *chunkCap: the frames of a render of nFrames per launch pair, at most;
// dFrameBuf is grown to hold them.
int growFrameBuf( pbr_ctx* ctx, uint32_t nFrames, size_t* chunkCap ) {
	const size_t pixelSlots = (size_t) ctx->numLocalTiles * 64;
	const size_t frameBytes = sizeof( float4 ) * pixelSlots;
	const size_t capFrames = std::max<size_t>( 1, kFrameBufBytes / frameBytes );
	size_t cap = std::min<size_t>( capFrames, nFrames );
	// the queue heads count pixel slots x frames of a band in 32 bits
	cap = std::min<size_t>( cap, std::max<size_t>( 1, 0x7FFFFFFFull / ( pixelSlots + 64 * (size_t) ctx->queueGrid.width ) ) );

	if( ctx->knobs.chunkFrames >= 1 ) {    // tests: force several launch pairs
		cap = std::min<size_t>( cap, (size_t) ctx->knobs.chunkFrames );
	}

	*chunkCap = cap;

	if( ctx->images.dFrameBuf.count() < pixelSlots * cap ) {
		// grown geometrically, never beyond the cap: at least 256 frames, then twice what is asked for.  A longer render
		// after a shorter one must not pay for a multi-GB reallocation inside every call (measured: 432 -> 512 frames at
		// 1080p, hipFree + hipMalloc of 16 GiB = 0.4 - 0.7 s when the pages have had other owners), and a small image must
		// not take 16 GiB because one render was longer than 256 frames (64 x 64 pixels, 300 frames: 39 MB).
		const size_t frames = std::min<size_t>( capFrames, std::max<size_t>( 256, ( cap <= 256 ) ? cap : 2 * cap ) );
		HIP_TRY( ctx, ctx->images.dFrameBuf.grow( pixelSlots * frames ) );
	}

	return PBR_OK;
}

// P deals the table `order` (device memory), whose bands' stretches start at first[]
void pointAtTable( DevParams* P, const unsigned* order, const unsigned* first ) {
	P->tileOrder = order;

	for( int band = 0; band < PT_BANDS; band++ ) {
		P->bandFirst[band] = first[band];
		P->bandTiles[band] = first[band + 1] - first[band];
	}
}

// The table a round of `tiles` tiles x `frames` frames is dealt from (pt_deal.hpp, dealRule); lastDeal names its order.
// settled: the schedule tuner has settled, or the plan is fixed.
const DealTable& dealOrder( pbr_ctx* ctx, size_t tiles, uint32_t frames, bool settled ) {
	const DealOrder dealt = dealRule( ctx->orderPinned, ctx->costLearnt, ctx->knobs.dealOrder, settled, ctx->cfg.tile_world > 1u, tiles, frames );
	std::snprintf( ctx->lastDeal, sizeof( ctx->lastDeal ), "%s", dealName( ctx->orderPinned, dealt ) );
	return ctx->images.deal[dealt];
}

// [1] the path loop (or a record slot of the asynchronous node phase that never filled), [2] a traversal that took more
// steps than the tree has nodes (PBR_GUARD builds): either way a walk was cut short and the image is wrong
int checkGuard( pbr_ctx* ctx ) {
	const volatile unsigned* guard = (const volatile unsigned*) ctx->dGuard;

	if( guard[1] != 0u || guard[2] != 0u ) {
		return fail( ctx, PBR_EDEVICE, "a bounded device loop of the path-tracing kernel gave up (path loop %u, traversal %u trips; pbr_diag_guard_trips): the image is incomplete",
		             guard[1], guard[2] );
	}

	if( guard[3] != 0u ) {
		return fail( ctx, PBR_EDEVICE, "the staged node prefix does not start at LDS address 0 (pt_kernel.hpp, stageHotNodes): this build of the kernels cannot be trusted" );
	}

	return PBR_OK;
}

// The focus chain of one launch of a chained render (pt_chain.hpp): the table is grown to the launch's frames, P is pointed at
// it, and the two kernels of the context's build flavour run ahead of the path-tracing launch.  prev: the image before the
// launch's first frame; first: the first launch of the render (tile sharding: the caller's distance starts the chain, the
// chain's own last value every launch after it).
typedef void ( *ChainPixelFn )( const ptk::DevParams, const float4*, float*, float*, int );
typedef void ( *ChainSlotsFn )( const ptk::DevParams, const float4*, float* );

int runFocusChain( pbr_ctx* ctx, DevParams* P, const float4* prev, bool first ) {
	const size_t pixelSlots = (size_t) ctx->numLocalTiles * 64;
	const size_t n = (size_t) P->nFrames;
	const size_t floats = pixelSlots * n + n;

	if( floats > 0xFFFFFFFFull ) {
		return fail( ctx, PBR_EINVAL, "focus chain: %zu pixel slots x %zu frames do not fit a 32-bit table index", pixelSlots, n );
	}

	if( ctx->images.dChain.count() < floats ) {
		// grown like the frame buffer whose quarter it is: at least 64 frames' worth, then twice what is asked for
		const size_t want = std::max<size_t>( ( pixelSlots + 1 ) * 64, ( n <= 64 ) ? floats : 2 * floats );
		HIP_TRY( ctx, ctx->images.dChain.grow( want ) );
	}

	// The main launch reads a pixel's 64 frames per wave (nextSlot), the chain writes a frame's 64 pixels per wave: layout 1
	// keeps a slot's frames side by side (one stretch per wave of the main launch), layout 0 a frame's slots (coalesced stores
	// here).  Measured at 1080p (profiles/r07/experiments/dof_render.txt): frame-major planes render the Cornell box's 256
	// frames in 116.8 ms against 121.1 ms (the chain alone 11.3 against 13.3 ms), the Sponza-class scene's 64 frames within
	// the spread of each other (chain 17.1 against 18.0 ms) — layout 0 it is.
	const bool slotMajor = ( ctx->knobs.chainLayout == 1 );
	P->chain = ctx->images.dChain;
	P->chainSlotStride = slotMajor ? (unsigned) n : 1u;
	P->chainFrameStride = slotMajor ? 1u : (unsigned) pixelSlots;
	P->chainFocusAt = (unsigned) ( pixelSlots * n );

	const int flavour = flavourOf( ctx->cfg );
	const pti_picker pick = kPickers[flavour][PTI_CHAIN];

	if( pick == nullptr ) {
		return fail( ctx, PBR_ESTATE, "this library was built without the focus chain of flavour %d", flavour );
	}

	const int lights = ( ctx->scene.numLights > 0 ) ? 1 : 0;
	const ChainPixelFn pixelKernel = (ChainPixelFn) pick( 0, 0, lights );
	const ChainSlotsFn slotsKernel = (ChainSlotsFn) pick( 1, 0, lights );
	DevParams C = *P;
	C.parkEighths = ( ctx->scene.numNodes >= kWideMinNodes ) ? 4 : 6;
	hipLaunchKernelGGL( pixelKernel, dim3( 1 ), dim3( 64 ), 0, ctx->stream, C, prev, ctx->images.dChain, ctx->dChainCarry, first ? 0 : 1 );
	HIP_TRY( ctx, hipGetLastError() );
	hipLaunchKernelGGL( slotsKernel, dim3( (unsigned) ( ( pixelSlots + 255 ) / 256 ) ), dim3( 256 ), 0, ctx->stream, C, prev, ctx->images.dChain );
	HIP_TRY( ctx, hipGetLastError() );
	return PBR_OK;
}

// What every render call starts with: the guard flags cleared, the call's seeds staged, the queue heads zero, and in P the scene
// and everything of the call that no launch of it changes.  focusGiven: the camera has a focus point and the caller passed the
// focus pixel's previous-frame distance (pbr_set_focus_depth) — consuming it is the caller's business.
int beginRender( pbr_ctx* ctx, const float* seeds, uint32_t nSeeds, const pbr_camera* cam, float pxDim, bool explicitWeight, float weight,
                 bool focusGiven, DevParams* out, uint32_t* hotAvail ) {
	// the kernels' error flags are of THIS render (host-mapped memory; no launch of this context is in flight here)
	for( int k = 0; k < 4; k++ ) {
		( (volatile unsigned*) ctx->dGuard )[k] = 0u;
	}

	PBR_TRY( stageSeeds( ctx, seeds, nSeeds ) );

	// the queue heads: foldFrames zeroes them behind every path-tracing launch, so only the first launch of a context
	// (and any launch after one that did not end in foldFrames) has to
	if( !ctx->workClean ) {
		HIP_TRY( ctx, hipMemsetAsync( ctx->dWork, 0, kWorkBytes, ctx->stream ) );
	}

	ctx->workClean = false;

	DevParams& P = *out;
	PBR_TRY( sceneParams( ctx, &P, hotAvail ) );   // P.nodes, P.firstRef / walkFirst for the configured traversal
	P.triPN = ctx->scene.dTriPN;
	P.phongAlpha = ctx->cfg.phong_tessellation;
	P.imgIn = ctx->images.dImgIn;
	P.imgOut = ctx->images.dImgOut;
	P.imgDbg = ctx->images.dImgDbg;
	P.counters = ctx->dCounters;
	P.workCounter = ctx->dWork;
	setCamera( &P, cam, (int) ctx->cfg.width, (int) ctx->cfg.height, pxDim );
	P.aperture = cam->lense[0] / cam->lense[1];
	P.samplesF = (float) ctx->cfg.samples;
	P.focusX = cam->focusPoint[0];
	P.focusY = cam->focusPoint[1];
	P.focusGiven = focusGiven ? 1 : 0;
	P.focusDepth = ctx->focusDepth;
	P.lenseFocal = cam->lense[0];
	P.lenseAperture = cam->lense[1];
	P.tilesX = ctx->tilesX;
	invariantDivisor( (unsigned) ctx->tilesX, P.tilesXDiv );
	P.numLocalTiles = ctx->numLocalTiles;
	P.tileWorld = (int) ctx->cfg.tile_world;
	P.tileRank = (int) ctx->cfg.tile_rank;
	P.maxDepth = (int) ctx->cfg.max_depth;
	P.maxAddedDepth = (int) ctx->cfg.max_added_depth;
	P.samples = (int) ctx->cfg.samples;
	P.useExplicitWeight = explicitWeight ? 1 : 0;
	P.explicitWeight = weight;
	P.antiAliasing = ctx->cfg.anti_aliasing;
	P.sky[0] = ctx->cfg.sky_light[0];
	P.sky[1] = ctx->cfg.sky_light[1];
	P.sky[2] = ctx->cfg.sky_light[2];
	return PBR_OK;
}

// ... and ends with, behind its last fold: the call's time on the device, and what the diagnostics report of its launches
int endRender( pbr_ctx* ctx, double traceMs, uint32_t launches ) {
	HIP_TRY( ctx, hipEventRecord( ctx->evStop, ctx->stream ) );
	PBR_TRY( timedTail( ctx ) );
	ctx->workClean = true;   // the last fold left the queue heads at zero
	ctx->lastTraceMs = traceMs;
	ctx->lastTraceLaunches = launches;
	return PBR_OK;
}

// chained: pbr_render_dof — many frames with depth of field in one call, the focus chain ahead of every launch
int launch( pbr_ctx* ctx, uint32_t firstCount, uint32_t nFrames, const float* seeds,
            bool explicitWeight, float weight, float pxDim, const pbr_camera* cam, bool chained = false ) {
	if( !ctx->hasScene || !ctx->configured ) {
		return fail( ctx, PBR_ESTATE, "render before pbr_upload_scene / pbr_configure" );
	}
	if( cam == nullptr || seeds == nullptr || nFrames == 0 ) {
		return fail( ctx, PBR_EINVAL, "render: null camera / seeds or zero frames" );
	}
	if( ctx->cfg.brdf != ctx->scene.sceneBrdf ) {
		return fail( ctx, PBR_EINVAL, "configured BRDF %u does not match the uploaded materials (BRDF %u)", ctx->cfg.brdf, ctx->scene.sceneBrdf );
	}

	const bool dof = ( cam->focusPoint[0] >= 0 && cam->focusPoint[1] >= 0 );

	if( dof && nFrames > 1 && !chained ) {
		return fail( ctx, PBR_EINVAL, "depth of field reads the previous frame of another pixel: render one frame per call" );
	}
	if( dof && ctx->cfg.tile_world > 1 && !ctx->focusGiven ) {
		return fail( ctx, PBR_EINVAL, "depth of field with tile sharding: the focus pixel's tile may live on another rank — pass its previous-frame distance with pbr_set_focus_depth (owner: pbr_get_focus_depth) before every %s", chained ? "pbr_render_dof call" : "frame" );
	}

	const bool chain = dof && chained;
	ctx->lastChainMs = 0.0;
	ctx->varianceCurrent = false;

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );

	DevParams P;
	uint32_t hotAvail = 0;
	PBR_TRY( beginRender( ctx, seeds, nFrames, cam, pxDim, explicitWeight, weight, dof && ctx->focusGiven, &P, &hotAvail ) );
	ctx->focusGiven = false;   // one frame's worth: the next frame needs the next distance

	const bool phong = ( ctx->cfg.phong_tessellation > 0.0f );

	if( phong && chain ) {
		return fail( ctx, PBR_EINVAL, "pbr_render_dof does not render Phong tessellation with a focus point (its plan has an intersection of its own); call pbr_render_frame + pbr_accumulate per frame" );
	}
	if( phong && ctx->scene.dTriPN == nullptr ) {
		return fail( ctx, PBR_EINVAL, "Phong tessellation needs a scene with usable vertex normals" );
	}

	PBR_TRY( buildPlans( ctx, hotAvail, phong, chain ) );
	size_t chunkCap = 0;
	PBR_TRY( growFrameBuf( ctx, nFrames, &chunkCap ) );
	ctx->tuner.beginRender( nFrames );

	// Phong tessellation has one plan; a pinned plan renders without tuning
	const Plan* plans = chain ? ctx->chainPlans : ctx->plans;   // the tuner's choice holds for both builds of a plan's kernel
	const Plan* forced = phong ? &ctx->phongPlan : ( ctx->pinnedPlan >= 0 ) ? &plans[std::min( ScheduleTuner::kPlans - 1, ctx->pinnedPlan )] : nullptr;
	const DealTable& table = dealOrder( ctx, (size_t) ctx->numLocalTiles, nFrames, forced != nullptr || ctx->tuner.settled() );
	pointAtTable( &P, table.dev, table.first );
	P.frameBuf = ctx->images.dFrameBuf;
	const size_t pixelSlots = (size_t) ctx->numLocalTiles * 64;
	P.frameStride = (unsigned) pixelSlots;
	const unsigned foldBlocks = (unsigned) ( ( pixelSlots + 255 ) / 256 );
	double traceMs = 0.0, chainMs = 0.0;
	uint32_t launches = 0, largest = 0;
	HIP_TRY( ctx, hipEventRecord( ctx->evStart, ctx->stream ) );

	for( uint32_t done = 0; done < nFrames; ) {
		// which plan renders this chunk, and how many frames of it
		const uint32_t most = std::min<uint32_t>( (uint32_t) chunkCap, nFrames - done );
		const Chunk chunk = ( forced != nullptr ) ? Chunk{ -1, most, -1, false } : ctx->tuner.next( most );
		const Plan& plan = ( forced != nullptr ) ? *forced : plans[chunk.plan];
		const uint32_t n = chunk.frames;
		P.nFrames = (int) n;
		invariantDivisor( n, P.framesDiv );
		P.firstCount = (int) ( firstCount + done );
		P.seeds = ctx->dSeeds + done;

		if( chain ) {
			// imageIn.w before the first launch, the last fold's .w — the previous launch's last first-hit distances — after it
			HIP_TRY( ctx, hipEventRecord( ctx->evChainStart, ctx->stream ) );
			PBR_TRY( runFocusChain( ctx, &P, done == 0 ? ctx->images.dImgIn : ctx->images.dImgOut, done == 0 ) );
		}

		HIP_TRY( ctx, hipEventRecord( ctx->evTraceStart, ctx->stream ) );
		PBR_TRY( runPlan( ctx, plan, &P, (size_t) ctx->numLocalTiles * n ) );
		HIP_TRY( ctx, hipEventRecord( ctx->evTraceStop, ctx->stream ) );
		// the running mean so far: the input image for the first chunk, imageOut after that
		hipLaunchKernelGGL( ptk::foldFrames, dim3( foldBlocks ), dim3( 256 ), 0, ctx->stream, P,
			(const float4*) ( done == 0 ? ctx->images.dImgIn : ctx->images.dImgOut ), ctx->images.dImgOut );
		HIP_TRY( ctx, hipGetLastError() );
		HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );   // one chunk for all but very long renders

		float ms = 0.0f;
		HIP_TRY( ctx, hipEventElapsedTime( &ms, ctx->evTraceStart, ctx->evTraceStop ) );
		traceMs += (double) ms;
		launches++;

		if( chain ) {
			float chainPart = 0.0f;
			HIP_TRY( ctx, hipEventElapsedTime( &chainPart, ctx->evChainStart, ctx->evTraceStart ) );
			chainMs += (double) chainPart;
		}

		if( n > largest ) {
			largest = n;
			std::snprintf( ctx->lastPlan, sizeof( ctx->lastPlan ), "%s", plan.name );
			std::snprintf( ctx->lastKernel, sizeof( ctx->lastKernel ), "%s", plan.kernelName );
		}

		ctx->tuner.record( chunk, (double) ms );
		done += n;
	}

	PBR_TRY( endRender( ctx, traceMs, launches ) );
	ctx->lastChainMs = chainMs;
	ctx->launchesSinceLearn += launches;
	PBR_TRY( checkGuard( ctx ) );
	return learnTileCosts( ctx, cam, pxDim );
}

// ---- pbr_render_adaptive: rounds of frames over the tiles that have not converged (pt_adaptive_host.hpp, pt_adaptive.hpp) ----
// The path-tracing kernels are launch()'s, untouched: a round is runPlan over a dealing table that names the active tiles only
// (nextSlot takes a band without tiles as exhausted; frameBufIndex, pixelOfSlot and the debug image work on the slot the
// table names), and foldFramesAdaptive folds and tests exactly those tiles.  numLocalTiles / frameStride stay the full values:
// they size the frame buffer.  The call neither feeds the schedule tuner nor the tile-cost learner, and the context's dealing
// tables stay as they are — the renders before and after it behave as if it had not been.

int launchAdaptive( pbr_ctx* ctx, uint32_t firstCount, const float* seeds, float pxDim, const pbr_camera* cam, const pbr_adaptive_params& A ) {
	if( !ctx->hasScene || !ctx->configured ) {
		return fail( ctx, PBR_ESTATE, "render before pbr_upload_scene / pbr_configure" );
	}
	if( ctx->cfg.brdf != ctx->scene.sceneBrdf ) {
		return fail( ctx, PBR_EINVAL, "configured BRDF %u does not match the uploaded materials (BRDF %u)", ctx->cfg.brdf, ctx->scene.sceneBrdf );
	}

	const bool phong = ( ctx->cfg.phong_tessellation > 0.0f );

	if( phong && ctx->scene.dTriPN == nullptr ) {
		return fail( ctx, PBR_EINVAL, "Phong tessellation needs a scene with usable vertex normals" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	const size_t tiles = (size_t) ctx->numLocalTiles;
	const size_t pixelSlots = tiles * 64;

	if( ctx->images.dMoments == nullptr ) {
		Images& I = ctx->images;
		const size_t perTile = std::max<size_t>( 1, tiles );
		HIP_TRY( ctx, allocAll( { want( I.dTileFrames, perTile ), want( I.dTileError, perTile ), want( I.dTileActive, perTile ), want( I.dAdaptiveOrder, perTile ),
		                          want( I.dMoments, std::max<size_t>( 1, pixelSlots ) ) } ) );
	}

	ctx->adaptiveStats = false;
	ctx->varianceCurrent = false;
	ctx->lastChainMs = 0.0;

	// the launch's parameters are launch()'s for a render without a focus point; a pending pbr_set_focus_depth stays pending
	DevParams P;
	uint32_t hotAvail = 0;
	PBR_TRY( beginRender( ctx, seeds, A.max_frames, cam, pxDim, false, 0.0f, false, &P, &hotAvail ) );

	PBR_TRY( buildPlans( ctx, hotAvail, phong, false ) );
	size_t chunkCap = 0;
	PBR_TRY( growFrameBuf( ctx, std::max( A.min_frames, std::min( A.round_frames, A.max_frames ) ), &chunkCap ) );

	// Phong tessellation has one plan; else the pinned plan, else what the tuner has kept, else phased-mid.  No tuning here: a
	// caller who wants the tuned plan renders with pbr_render first.
	const int kPhasedMid = 4;
	const Plan& plan = phong ? ctx->phongPlan
	                   : ( ctx->pinnedPlan >= 0 ) ? ctx->plans[std::min( ScheduleTuner::kPlans - 1, ctx->pinnedPlan )]
	                   : ctx->plans[ctx->tuner.settled() ? ctx->tuner.tunedPlan() : kPhasedMid];
	std::snprintf( ctx->lastPlan, sizeof( ctx->lastPlan ), "%s", plan.name );
	std::snprintf( ctx->lastKernel, sizeof( ctx->lastKernel ), "%s", plan.kernelName );

	P.frameBuf = ctx->images.dFrameBuf;
	P.frameStride = (unsigned) pixelSlots;

	const std::vector<AdaptivePair> pairs = adaptiveSchedule( A.min_frames, A.round_frames, A.max_frames, (uint32_t) chunkCap );
	std::vector<unsigned> active( tiles, 1u ), order;
	unsigned first[PT_BANDS + 1];
	size_t activeTiles = tiles;
	const unsigned* dTable = nullptr;   // the round's dealing table = the list of its tiles
	double traceMs = 0.0, foldMs = 0.0;
	uint32_t launches = 0, rounds = 0;
	uint64_t units = 0;
	bool roundStart = true;
	HIP_TRY( ctx, hipEventRecord( ctx->evStart, ctx->stream ) );

	for( size_t at = 0; at < pairs.size() && activeTiles > 0; at++ ) {
		const AdaptivePair& pair = pairs[at];

		if( roundStart ) {
			// the round's frames (its pairs up to the one that ends it) decide the table, the active tiles are filtered from it
			uint32_t roundFrames = 0;

			for( size_t k = at; k < pairs.size(); k++ ) {
				roundFrames += pairs[k].frames;

				if( pairs[k].endsRound ) {
					break;
				}
			}

			const DealTable& table = dealOrder( ctx, activeTiles, roundFrames, true );   // the plan is fixed

			if( activeTiles == tiles ) {
				dTable = table.dev;
				std::copy( table.first, table.first + PT_BANDS + 1, first );
			}
			else {
				filterOrder( table.host, table.first, active.data(), PT_BANDS, &order, first );
				HIP_TRY( ctx, hipMemcpyAsync( ctx->images.dAdaptiveOrder, order.data(), sizeof( unsigned ) * order.size(), hipMemcpyHostToDevice, ctx->stream ) );
				HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );   // the source is pageable
				dTable = ctx->images.dAdaptiveOrder;
			}

			if( (size_t) first[PT_BANDS] != activeTiles ) {
				return fail( ctx, PBR_ESTATE, "pbr_render_adaptive: the dealing table names %u of %zu active tiles", first[PT_BANDS], activeTiles );
			}

			pointAtTable( &P, dTable, first );
			roundStart = false;
		}

		const uint32_t n = pair.frames;
		P.nFrames = (int) n;
		invariantDivisor( n, P.framesDiv );
		P.firstCount = (int) ( firstCount + pair.first );
		P.seeds = ctx->dSeeds + pair.first;

		HIP_TRY( ctx, hipEventRecord( ctx->evTraceStart, ctx->stream ) );
		PBR_TRY( runPlan( ctx, plan, &P, activeTiles * n ) );
		HIP_TRY( ctx, hipEventRecord( ctx->evTraceStop, ctx->stream ) );
		// the running mean so far: the input image for the first pair (every tile is in it), imageOut after that
		HIP_TRY( ctx, hipEventRecord( ctx->evFoldStart, ctx->stream ) );
		hipLaunchKernelGGL( ptk::foldFramesAdaptive, dim3( (unsigned) ( ( activeTiles + 3 ) / 4 ) ), dim3( 256 ), 0, ctx->stream, P,
			(const float4*) ( pair.first == 0 ? ctx->images.dImgIn : ctx->images.dImgOut ), ctx->images.dImgOut, dTable, (unsigned) activeTiles,
			ctx->images.dMoments, pair.first, pair.endsRound ? 1 : 0, A.threshold, ctx->images.dTileFrames, ctx->images.dTileError, ctx->images.dTileActive );
		HIP_TRY( ctx, hipGetLastError() );
		HIP_TRY( ctx, hipEventRecord( ctx->evFoldStop, ctx->stream ) );

		if( pair.endsRound ) {
			HIP_TRY( ctx, hipMemcpyAsync( active.data(), ctx->images.dTileActive, sizeof( unsigned ) * tiles, hipMemcpyDeviceToHost, ctx->stream ) );
		}

		HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );

		float ms = 0.0f;
		HIP_TRY( ctx, hipEventElapsedTime( &ms, ctx->evTraceStart, ctx->evTraceStop ) );
		traceMs += (double) ms;
		HIP_TRY( ctx, hipEventElapsedTime( &ms, ctx->evFoldStart, ctx->evFoldStop ) );
		foldMs += (double) ms;
		launches++;
		units += (uint64_t) activeTiles * 64u * n;

		if( pair.endsRound ) {
			rounds++;
			activeTiles = 0;

			for( size_t t = 0; t < tiles; t++ ) {
				activeTiles += ( active[t] != 0u ) ? 1u : 0u;
			}

			roundStart = true;
		}
	}

	PBR_TRY( endRender( ctx, traceMs, launches ) );
	ctx->lastAdaptiveRounds = rounds;
	ctx->lastAdaptiveUnits = units;
	ctx->lastAdaptiveFoldMs = foldMs;
	ctx->adaptiveStats = true;
	return checkGuard( ctx );
}

int readTiled( pbr_ctx* ctx, const float4* tiles, float* rgba, int tileWorld, int tileRank ) {
	if( !ctx->configured || tiles == nullptr ) {
		return fail( ctx, PBR_ESTATE, "read before pbr_configure (or before pbr_import_tiles)" );
	}
	if( rgba == nullptr ) {
		return fail( ctx, PBR_EINVAL, "read: null destination" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	hipLaunchKernelGGL( ptk::untile, imageGrid( (int) ctx->cfg.width, (int) ctx->cfg.height ), kImageBlock, 0, ctx->stream, tiles, ctx->images.dRows,
		(int) ctx->cfg.width, (int) ctx->cfg.height, ctx->tilesX, tileWorld, tileRank );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipMemcpyAsync( rgba, ctx->images.dRows, sizeof( float4 ) * ctx->cfg.width * ctx->cfg.height, hipMemcpyDeviceToHost, ctx->stream ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	return PBR_OK;
}

}  // namespace


extern "C" {

uint32_t pbr_abi_version( void ) {
	return PBR_ABI_VERSION;
}

int pbr_mode_built( uint32_t traversal, uint32_t arith ) {
	if( traversal > 3 || arith > 1 ) {
		return -1;
	}

	const int flavour = flavourOf( traversal, arith );

	for( int group = 0; group < PTI_GROUPS; group++ ) {
		// builds without the hand-scheduled node phase, and the compact record's flavours, have no two-paths kernels
		if( group == PTI_DUAL && !dualIsDual( flavour ) ) {
			continue;
		}
		if( kPickers[flavour][group] == nullptr ) {
			return 0;
		}
		if( group != PTI_REFILL_PHONG && group != PTI_CHAIN && group != PTI_WALK && kPickers[flavour | PTI_CHAINED][group] == nullptr ) {
			return 0;
		}
	}

	return 1;
}

int pbr_create( int device, pbr_ctx** out ) {
	if( out == nullptr ) {
		return PBR_EINVAL;
	}

	pbr_ctx* ctx = new pbr_ctx();
	*out = ctx;
	ctx->device = device;

	int count = 0;
	hipError_t err = hipGetDeviceCount( &count );

	if( err != hipSuccess || count <= 0 ) {
		return fail( ctx, PBR_EDEVICE, "no HIP device available (%s); this library has no CPU path", hipGetErrorString( err ) );
	}
	if( device < 0 || device >= count ) {
		return fail( ctx, PBR_EINVAL, "device %d out of range (%d devices)", device, count );
	}

	HIP_TRY( ctx, hipSetDevice( device ) );
	hipDeviceProp_t prop;
	HIP_TRY( ctx, hipGetDeviceProperties( &prop, device ) );
	ctx->numCUs = prop.multiProcessorCount;
	HIP_TRY( ctx, hipStreamCreateWithFlags( &ctx->stream.s, hipStreamNonBlocking ) );

	for( Event* event : { &ctx->evStart, &ctx->evTraceStart, &ctx->evTraceStop, &ctx->evStop, &ctx->evChainStart, &ctx->evFoldStart, &ctx->evFoldStop,
	                      &ctx->evRelinkStart, &ctx->evRelinkStop, &ctx->evXfStart, &ctx->evXfStop, &ctx->evXfNormalsStart, &ctx->evXfNormalsStop,
	                      &ctx->evHistogramStart, &ctx->evHistogramStop } ) {
		HIP_TRY( ctx, hipEventCreate( &event->e ) );
	}

	HIP_TRY( ctx, ctx->dChainCarry.alloc( 1 ) );
	HIP_TRY( ctx, ctx->dCounters.alloc( kCounterSlots ) );
	HIP_TRY( ctx, ctx->dWork.alloc( kWorkBytes / sizeof( unsigned int ) ) );
	// host-visible so that it can be read while a kernel is still running
	HIP_TRY( ctx, hipHostMalloc( (void**) &ctx->dGuard, sizeof( unsigned int ) * 4, hipHostMallocMapped ) );
	std::memset( ctx->dGuard, 0, sizeof( unsigned int ) * 4 );
	HIP_TRY( ctx, hipMemset( ctx->dCounters, 0, sizeof( unsigned long long ) * kCounterSlots ) );

	return PBR_OK;
}

void pbr_destroy( pbr_ctx* ctx ) {
	if( ctx == nullptr ) {
		return;
	}

	if( ctx->stream != nullptr ) {
		(void) hipSetDevice( ctx->device );
		(void) hipStreamSynchronize( ctx->stream );
		(void) hipHostFree( ctx->dGuard );
	}

	// the buffers, then the events, then the stream: the order the context declares them in, backwards
	delete ctx;
}

const char* pbr_last_error( const pbr_ctx* ctx ) {
	return ( ctx != nullptr ) ? ctx->error.c_str() : "null context";
}

int pbr_validate_scene( const pbr_scene_desc* s, char* message, size_t capacity ) {
	std::string why;
	const int status = checkScene( s, nullptr, &why );

	if( message != nullptr && capacity > 0 ) {
		std::snprintf( message, capacity, "%s", why.c_str() );
	}

	return status;
}

int pbr_upload_scene( pbr_ctx* ctx, const pbr_scene_desc* s ) {
	if( ctx == nullptr || ctx->stream == nullptr ) {
		return fail( ctx, PBR_ESTATE, "context is not usable" );
	}

	// everything on the host first — the scene, and the records of a ray-ordered walk the context is configured for — so
	// that a scene the walk cannot take leaves the context as it was
	SceneTree tree;
	PackedScene packed;
	PackedWalk walk;
	PBR_TRY( checkScene( s, &tree, &ctx->error ) );
	PBR_TRY( packScene( s, tree, &packed, &ctx->error ) );
	RefitPlan refit;
	planRefit( tree, packed.nodes.recordOf, kRefitSubtree, &refit );   // a tree that cannot be refitted uploads all the same: refit.why

	if( ctx->configured ) {
		PBR_TRY( packConfiguredWalk( ctx, ctx->cfg, &tree, &walk ) );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	freeScene( ctx );
	ctx->temporal.drop();   // pbr_denoise_temporal: the history's features are the old scene's

	auto toDevice = [ctx]( Owned<float4>* dst, const std::vector<Quad>& src ) {
		HIP_TRY( ctx, dst->alloc( src.size() ) );
		HIP_TRY( ctx, hipMemcpy( dst->get(), src.data(), sizeof( Quad ) * src.size(), hipMemcpyHostToDevice ) );
		return PBR_OK;
	};

	PBR_TRY( toDevice( &ctx->scene.dNodes, packed.nodes.storage ) );
	PBR_TRY( toDevice( &ctx->scene.dTris, packed.tris ) );

	if( !packed.triPN.empty() ) {
		PBR_TRY( toDevice( &ctx->scene.dTriPN, packed.triPN ) );
		// pbr_update_geometry gathers the patches again: the indices and the normals wait on the host for its first call
		ctx->scene.patchFacesN.assign( s->facesN, s->facesN + s->num_faces );
		ctx->scene.patchNormals.assign( s->normals, s->normals + s->num_normals );
	}

	ctx->scene.numNormals = s->num_normals;

	PBR_TRY( toDevice( &ctx->scene.dMats, packed.mats ) );
	PBR_TRY( toDevice( &ctx->scene.dLights, packed.lights ) );

	// the face normals the shading would recompute on every hit, evaluated once by the shading's own device function
	if( s->num_faces > 0 && ctx->knobs.faceNormals != 0 ) {
		HIP_TRY( ctx, ctx->scene.dFaceN.alloc( s->num_faces ) );
		DevParams P;
		std::memset( &P, 0, sizeof( P ) );
		P.tris = ctx->scene.dTris;
		hipLaunchKernelGGL( ptk::prepareFaceNormals, dim3( ( s->num_faces + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, P, ctx->scene.dFaceN, (int) s->num_faces );
		HIP_TRY( ctx, hipGetLastError() );
	}

	// what pbr_update_vertices needs on the device (its bytes: Scene::refitBytes)
	auto keep = [ctx]( auto* dst, const void* src, size_t count ) {
		HIP_TRY( ctx, dst->alloc( count ) );

		if( src != nullptr && count > 0 ) {
			HIP_TRY( ctx, hipMemcpy( dst->get(), src, dst->bytes(), hipMemcpyHostToDevice ) );
		}

		return PBR_OK;
	};
	Scene& S = ctx->scene;
	PBR_TRY( keep( &S.dVertices, s->vertices, s->num_vertices ) );   // the positions a first update's motion starts from; pbr_read_geometry's, refit or not

	if( refit.nested ) {
		const Quad rootBox[2] = { { s->bvh[0].bbMin.x, s->bvh[0].bbMin.y, s->bvh[0].bbMin.z, -1.0f }, { s->bvh[0].bbMax.x, s->bvh[0].bbMax.y, s->bvh[0].bbMax.z, -1.0f } };
		PBR_TRY( keep( &S.dFacesV, s->facesV, s->num_faces ) );
		PBR_TRY( keep( &S.dRootBox, rootBox, 2 ) );
		PBR_TRY( keep( &S.dRefitSlots, refit.slots.data(), refit.slots.size() ) );
		PBR_TRY( keep( &S.dRefitInfo, refit.info.data(), refit.info.size() ) );
		PBR_TRY( keep( &S.dRefitHeights, refit.height16.data(), refit.height16.size() ) );
		PBR_TRY( keep( &S.dRefitRecordOf, refit.recordOf.data(), refit.recordOf.size() ) );
		PBR_TRY( keep( &S.dRefitTop, refit.topNodes.data(), refit.topNodes.size() ) );
		PBR_TRY( keep( &S.dRefitLevelFirst, refit.topLevelFirst.data(), refit.topLevelFirst.size() ) );
	}

	S.refitGroups = refit.numGroups();
	S.refitLevels = refit.numLevels();
	S.refitTopNodes = (uint32_t) refit.topNodes.size();
	S.refitSubtrees = (uint32_t) refit.subtreeRoots.size();
	S.numVertices = s->num_vertices;
	// the host keeps the verdict and node -> record; the rest is on the device now
	for( std::vector<uint32_t>* v : { &refit.parent, &refit.end, &refit.height, &refit.subtreeRoots, &refit.groupFirst, &refit.slots, &refit.topNodes, &refit.topLevelFirst, &refit.info } ) {
		std::vector<uint32_t>().swap( *v );
	}
	std::vector<uint16_t>().swap( refit.height16 );
	ctx->scene.refit = std::move( refit );

	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	ctx->scene.numHotAvail = packed.nodes.hotSlots;
	ctx->scene.firstRef = packed.nodes.first[0];
	ctx->scene.tree = std::move( tree );
	ctx->scene.numNodes = s->num_nodes;
	ctx->scene.numFaces = s->num_faces;
	ctx->scene.numMaterials = s->num_materials;
	ctx->scene.numLights = s->num_lights;
	ctx->scene.sceneBrdf = s->brdf;
	replan( ctx );   // a new scene / configuration is tuned afresh
	ctx->hasScene = true;

	return walk.storage.empty() ? PBR_OK : uploadWalkStreams( ctx, walk, ctx->cfg.traversal );
}

namespace {

// The re-link's tables for the layout dNodesWalk holds (pt_relink_host.hpp, relinkTables): built from the host copy of the tree —
// its shape and the ranking of the upload; the boxes are not read — on the first re-linked update after the streams were built,
// kept until the streams go.  Nothing of the context changes when this fails.
int ensureRelinkTables( pbr_ctx* ctx ) {
	if( ctx->scene.walk.dRelink != nullptr ) {
		return PBR_OK;
	}

	RefitPlan shape;
	RelinkTables t;
	refitNesting( ctx->scene.tree, &shape );
	PBR_TRY( relinkTables( ctx->scene.tree, shape, ctx->scene.walk.walkBuilt, &t, &ctx->error ) );

	if( sizeof( Quad ) * t.storageQuads != ctx->scene.walk.dNodesWalk.bytes() ) {
		return fail( ctx, PBR_ESTATE, "pbr_update_vertices: the re-link expects %zu bytes of records, the streams hold %llu", sizeof( Quad ) * t.storageQuads, (unsigned long long) ctx->scene.walk.dNodesWalk.bytes() );
	}

	// one allocation, every table on a 256-byte boundary
	size_t bytes = 0;
	auto place = [&bytes]( size_t size ) {
		const size_t at = bytes;
		bytes += ( size + 255 ) & ~(size_t) 255;
		return at;
	};
	const size_t N = t.N;
	const size_t atRank = place( sizeof( uint32_t ) * N ), atCold = place( sizeof( uint32_t ) * ( N + 1 ) ), atBase = place( sizeof( uint32_t ) * N );
	const size_t atNodes = place( sizeof( uint32_t ) * t.levelNodes.size() ), atFirst = place( sizeof( uint32_t ) * t.levelFirst.size() );
	const size_t atAxis = place( N ), atPerm = place( sizeof( uint32_t ) * t.permEntries() );
	const size_t atNext = place( sizeof( int ) * t.nextEntries() ), atPos = place( sizeof( uint32_t ) * t.posEntries() );

	Owned<unsigned char> owner;
	HIP_TRY( ctx, owner.alloc( bytes ) );
	unsigned char* const slab = owner.get();
	hipError_t err = hipMemset( slab, 0, bytes );
	auto put = [&]( size_t at, const std::vector<uint32_t>& src ) {
		err = ( err != hipSuccess ) ? err : hipMemcpy( slab + at, src.data(), sizeof( uint32_t ) * src.size(), hipMemcpyHostToDevice );
	};
	put( atRank, t.rankOf );
	put( atCold, t.coldBefore );
	put( atBase, t.childBase );
	put( atNodes, t.levelNodes );
	put( atFirst, t.levelFirst );
	err = ( err != hipSuccess ) ? err : hipDeviceSynchronize();   // the memset ran on the null stream; launches use ctx->stream

	if( err != hipSuccess ) {
		return fail( ctx, PBR_EDEVICE, "pbr_update_vertices: the re-link's tables: %s", hipGetErrorString( err ) );
	}

	RelinkView& v = ctx->scene.walk.relinkView;
	v.N = t.N;
	v.scheme = t.scheme;
	v.compact = t.compact;
	v.K = t.K;
	v.V = t.V;
	v.streams = t.streams;
	v.hotPerStream = t.hotPerStream;
	v.rankOf = (const uint32_t*) ( slab + atRank );
	v.coldBefore = (const uint32_t*) ( slab + atCold );
	v.childBase = (const uint32_t*) ( slab + atBase );
	v.axis = (unsigned char*) ( slab + atAxis );
	v.perm = (uint32_t*) ( slab + atPerm );
	v.next = (int*) ( slab + atNext );
	v.pos = (uint32_t*) ( slab + atPos );
	ctx->scene.walk.dRelinkLevelNodes = (unsigned*) ( slab + atNodes );
	ctx->scene.walk.dRelinkLevelFirst = (unsigned*) ( slab + atFirst );
	ctx->scene.walk.relinkRuns = t.runs;
	ctx->scene.walk.relinkLevels = t.numLevels();
	ctx->scene.walk.relinkContainers = (uint32_t) t.levelNodes.size();
	ctx->scene.walk.dRelink = std::move( owner );
	return PBR_OK;
}

// The re-link's launches on the context's stream, behind the refit's: sort, the levels top-down, the records.
int launchRelink( pbr_ctx* ctx ) {
	RelinkView v = ctx->scene.walk.relinkView;
	v.refNodes = (const RelinkQuad*) ctx->scene.dNodes.get();
	v.refRecordOf = ctx->scene.dRefitRecordOf;
	v.info = ctx->scene.dRefitInfo;
	v.header = (int*) ctx->scene.walk.dNodesWalk.get();
	v.records = (RelinkQuad*) ( ctx->scene.walk.dNodesWalk + 2 );
	uint32_t launches = 0;
	HIP_TRY( ctx, hipEventRecord( ctx->evRelinkStart, ctx->stream ) );
	hipLaunchKernelGGL( ptl::relinkSortKernel, dim3( ( ctx->scene.walk.relinkContainers + RELINK_THREADS - 1 ) / RELINK_THREADS ), dim3( RELINK_THREADS ), 0, ctx->stream,
	                    v, ctx->scene.walk.dRelinkLevelNodes, ctx->scene.walk.relinkContainers );
	HIP_TRY( ctx, hipGetLastError() );
	launches++;

	for( const RelinkRun& run : ctx->scene.walk.relinkRuns ) {
		hipLaunchKernelGGL( ptl::relinkLevelsKernel, dim3( run.blocks ), dim3( run.threads ), 0, ctx->stream,
		                    v, ctx->scene.walk.dRelinkLevelNodes, ctx->scene.walk.dRelinkLevelFirst, run.firstLevel, run.numLevels );
		HIP_TRY( ctx, hipGetLastError() );
		launches++;
	}

	hipLaunchKernelGGL( ptl::relinkRecordsKernel, dim3( ( v.N - 1 + RELINK_THREADS - 1 ) / RELINK_THREADS, v.streams ), dim3( RELINK_THREADS ), 0, ctx->stream, v );
	HIP_TRY( ctx, hipGetLastError() );
	launches++;
	HIP_TRY( ctx, hipEventRecord( ctx->evRelinkStop, ctx->stream ) );
	ctx->lastRelinkLaunches = launches;
	return PBR_OK;
}

}  // namespace

int pbr_refit_ordered_walk( pbr_ctx* ctx, int on ) {
	PBR_TRY( usable( ctx ) );

	ctx->refitOrdered = ( on != 0 );
	return PBR_OK;
}

namespace {

// The device tables of pbr_update_geometry, made by the first such call after an upload from the host copies the upload kept:
// the faces' normal indices, the vertex normals, and the scratch table of the faces' thick boxes.  Nothing of the context
// changes when this fails.
int ensurePatchTables( pbr_ctx* ctx ) {
	if( ctx->scene.dFaceBoxes != nullptr ) {
		return PBR_OK;
	}

	Scene& S = ctx->scene;
	Owned<uint4> indices;
	Owned<float4> normals;
	Owned<float2> boxes;   // six floats per face
	hipError_t err = (hipError_t) allocAll( { want( indices, S.patchFacesN.size() ), want( normals, S.patchNormals.size() ), want( boxes, 3 * (size_t) S.numFaces ) } );
	err = ( err != hipSuccess ) ? err : hipMemcpy( indices, S.patchFacesN.data(), indices.bytes(), hipMemcpyHostToDevice );
	err = ( err != hipSuccess ) ? err : hipMemcpy( normals, S.patchNormals.data(), normals.bytes(), hipMemcpyHostToDevice );

	if( err != hipSuccess ) {
		return fail( ctx, PBR_EDEVICE, "pbr_update_geometry: the patch refit's tables: %s", hipGetErrorString( err ) );
	}

	S.dPatchFacesN = std::move( indices );
	S.dPatchNormals = std::move( normals );
	S.dFaceBoxes = std::move( boxes );
	std::vector<pbr_uint4>().swap( S.patchFacesN );   // the device holds them now
	std::vector<pbr_float4>().swap( S.patchNormals );
	return PBR_OK;
}

// One update call: its kind, and what that kind brings.
struct UpdateCall {
	UpdateKind kind;
	const pbr_float4* vertices;   // Vertices, Geometry: V'
	uint32_t num_vertices;
	const pbr_float4* normals;    // Geometry: N', or NULL and 0 to keep the context's
	uint32_t num_normals;
	const float* weights;         // Morph, Pose: one per target
	uint32_t num_targets;
	const float* matrices;        // Transforms: one per part; Skin, Pose: one per bone; SkinDQ, PoseDQ: one dual quaternion per bone
	uint32_t num_matrices;
};

// pbr_denoise_temporal under motion tracking: H, the positions the history was made under, is a copy of dVertices taken before
// an update replaces them.  The copy runs on the stream and is waited for.
int keepHistoryVertices( pbr_ctx* ctx, const char* call ) {
	hipError_t kept = (hipError_t) ctx->scene.dHistVertices.grow( ctx->scene.numVertices );
	kept = ( kept != hipSuccess ) ? kept : hipMemcpyAsync( ctx->scene.dHistVertices, ctx->scene.dVertices, sizeof( pbr_float4 ) * ctx->scene.numVertices, hipMemcpyDeviceToDevice, ctx->stream );
	kept = ( kept != hipSuccess ) ? kept : hipStreamSynchronize( ctx->stream );

	if( kept != hipSuccess ) {
		ctx->temporal.drop();
		return fail( ctx, PBR_EDEVICE, "%s: keeping the history's vertex positions: %s", call, hipGetErrorString( kept ) );
	}

	return PBR_OK;
}

// What pt_update_host.hpp's decisions read of the context.  (It returns a C++ struct, so it steps out of the C linkage.)
extern "C++" UpdateFacts updateFacts( const pbr_ctx* ctx ) {
	UpdateFacts f;
	f.hasScene = ctx->hasScene;
	f.nested = ctx->scene.refit.nested;
	f.why = ctx->scene.refit.why.c_str();
	f.configured = ctx->configured;
	f.traversal = ctx->cfg.traversal;
	f.phongTessellation = ctx->cfg.phong_tessellation;
	f.refitOrdered = ctx->refitOrdered;
	f.hasPatches = ( ctx->scene.dTriPN != nullptr );
	f.walkBuilt = ( ctx->scene.walk.dNodesWalk != nullptr && ctx->scene.walk.walkBuilt == ctx->cfg.traversal );
	f.numParts = ctx->scene.parts.count;
	f.numBones = ctx->scene.skin.count;
	f.numMorphTargets = ctx->scene.morph.count;
	f.skinGeneration = ctx->scene.skin.pose.generation;
	f.morphGeneration = ctx->scene.morph.pose.generation;
	f.partNormals = ctx->scene.parts.pose.normals;
	f.skinNormals = ctx->scene.skin.pose.normals;
	f.morphNormals = ctx->scene.morph.pose.normals;
	f.tracking = ctx->temporal.tracking;
	f.history = ctx->temporal.history;
	f.moved = ctx->temporal.moved;
	return f;
}

// The kind's argument check (stage 2 of pt_update_host.hpp); it fills the pinned tables the update uploads.
int checkUpdateArguments( pbr_ctx* ctx, const UpdateCall& u, const char* call ) {
	switch( u.kind ) {
		case UpdateKind::Pose:
			PBR_TRY( checkMorphWeights( u.weights, u.num_targets, ctx->scene.morph.count, ctx->scene.morph.hWeights, &ctx->error, call ) );
			return checkSkinMatrices( u.matrices, u.num_matrices, ctx->scene.skin.count, ctx->scene.skin.hBones, &ctx->error, call );

		case UpdateKind::Morph:
			return checkMorphWeights( u.weights, u.num_targets, ctx->scene.morph.count, ctx->scene.morph.hWeights, &ctx->error, call );

		case UpdateKind::Skin:
			return checkSkinMatrices( u.matrices, u.num_matrices, ctx->scene.skin.count, ctx->scene.skin.hBones, &ctx->error, call );

		case UpdateKind::PoseDQ:
			PBR_TRY( checkMorphWeights( u.weights, u.num_targets, ctx->scene.morph.count, ctx->scene.morph.hWeights, &ctx->error, call ) );
			return checkSkinDualQuats( u.matrices, u.num_matrices, ctx->scene.skin.count, ctx->scene.skin.hBones, &ctx->error, call );

		case UpdateKind::SkinDQ:
			return checkSkinDualQuats( u.matrices, u.num_matrices, ctx->scene.skin.count, ctx->scene.skin.hBones, &ctx->error, call );

		case UpdateKind::Transforms:
			return checkTransforms( u.matrices, u.num_matrices, ctx->scene.parts.count, ctx->scene.parts.hRecords, &ctx->error );

		case UpdateKind::Geometry:
			PBR_TRY( checkRefitVertices( u.vertices, u.num_vertices, ctx->scene.numVertices, &ctx->error, call ) );
			return checkRefitNormals( u.normals, u.num_normals, ctx->scene.numNormals, &ctx->error );

		default:
			return checkRefitVertices( u.vertices, u.num_vertices, ctx->scene.numVertices, &ctx->error, call );
	}
}

// The rest pose an update of this kind starts from, and whose statistics it moves; none for the kinds that bring V' from the host.
RestPose* restPoseOf( pbr_ctx* ctx, UpdateKind kind ) {
	switch( kind ) {
		case UpdateKind::Transforms: return &ctx->scene.parts.pose;
		case UpdateKind::Skin:
		case UpdateKind::SkinDQ: return &ctx->scene.skin.pose;
		case UpdateKind::Morph:
		case UpdateKind::Pose:
		case UpdateKind::PoseDQ: return &ctx->scene.morph.pose;
		default: return nullptr;
	}
}

// The sequence every kind that computes V' on the device goes through, once: H first (pbr_denoise_temporal under motion
// tracking: a copy nobody reads if the call is refused), `upload` (the call's tables, asynchronous copies on the stream), the
// flag word cleared, `launch` (the kernel that writes V' to the pose's staging buffer and raises the flag word for a position
// that is not finite — finite arguments can overflow, and the host never sees V') between evXfStart and evXfStop, the flag's 4
// bytes read back — and only then the temporal policy hears of an update and the staging buffer becomes the context's vertices
// (the two pointers are swapped).  A refused call leaves the context as it was.  The normals cannot fail; the caller writes them
// after this returns PBR_OK.  (A template, so it steps out of the C linkage this part of the file is in.)
extern "C++" template<class Upload, class Launch>
int stageVertices( pbr_ctx* ctx, const char* call, RestPose* pose, bool keepsHistory, const char* overflow, Upload upload, Launch launch ) {
	if( keepsHistory ) {
		PBR_TRY( keepHistoryVertices( ctx, call ) );
	}

	const auto uploadStart = std::chrono::steady_clock::now();
	*pose->hFlag = 0u;
	HIP_TRY( ctx, upload() );
	HIP_TRY( ctx, hipMemcpyAsync( pose->dFlag, pose->hFlag, sizeof( unsigned ), hipMemcpyHostToDevice, ctx->stream ) );
	const double uploadMs = std::chrono::duration<double, std::milli>( std::chrono::steady_clock::now() - uploadStart ).count();
	HIP_TRY( ctx, hipEventRecord( ctx->evStart, ctx->stream ) );
	HIP_TRY( ctx, hipEventRecord( ctx->evXfStart, ctx->stream ) );
	launch();
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipEventRecord( ctx->evXfStop, ctx->stream ) );
	HIP_TRY( ctx, hipMemcpyAsync( pose->hFlag, pose->dFlag, sizeof( unsigned ), hipMemcpyDeviceToHost, ctx->stream ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );

	if( *pose->hFlag != 0u ) {
		return fail( ctx, PBR_EINVAL, "%s: %s", call, overflow );
	}

	ctx->temporal.update();   // the H it asks for is kept already
	ctx->scene.dVertices.swap( pose->dStaged );
	ctx->lastRefitUploadMs = uploadMs;
	return PBR_OK;
}

// V' of a kind that computes it on the device: the kind's tables, its kernel and its overflow message through stageVertices.
int stageKind( pbr_ctx* ctx, UpdateKind kind, const char* call, bool keepsHistory ) {
	const uint32_t V = ctx->scene.numVertices;
	const dim3 grid( ( V + 255 ) / 256 ), group( 256 );
	PartsState& parts = ctx->scene.parts;
	SkinState& skin = ctx->scene.skin;
	MorphState& morph = ctx->scene.morph;
	const auto uploadBones = [&]() { return hipMemcpyAsync( skin.dBones, skin.hBones, sizeof( pbr_float4 ) * 3 * skin.count, hipMemcpyHostToDevice, ctx->stream ); };
	// the dual quaternions of the two dq kinds lie in the same tables, two quads per bone
	const auto uploadDualQuats = [&]() { return hipMemcpyAsync( skin.dBones, skin.hBones, sizeof( pbr_float4 ) * 2 * skin.count, hipMemcpyHostToDevice, ctx->stream ); };
	const auto uploadWeights = [&]() { return hipMemcpyAsync( morph.dWeights, morph.hWeights, sizeof( float ) * morph.count, hipMemcpyHostToDevice, ctx->stream ); };

	switch( kind ) {
		case UpdateKind::Transforms:
			return stageVertices( ctx, call, &parts.pose, keepsHistory, "a transformed position is not finite (the matrices are finite, their product with the rest pose overflows; found on the device)",
			                      [&]() { return hipMemcpyAsync( parts.dRecords, parts.hRecords, sizeof( ptx::PartRecord ) * parts.count, hipMemcpyHostToDevice, ctx->stream ); },
			                      [&]() { hipLaunchKernelGGL( ptr::transformVertices, grid, group, 0, ctx->stream, parts.pose.dRest, parts.dOfVertex, parts.dRecords, parts.pose.dStaged, parts.pose.dFlag, (int) V ); } );

		case UpdateKind::Skin:
			return stageVertices( ctx, call, &skin.pose, keepsHistory, "a skinned position is not finite (the matrices are finite, their blend's product with the rest pose overflows; found on the device)",
			                      uploadBones,
			                      [&]() { hipLaunchKernelGGL( ptr::skinVertices, grid, group, 0, ctx->stream, skin.pose.dRest, skin.dOfVertex, skin.dBones, skin.pose.dStaged, skin.pose.dFlag, (int) V ); } );

		case UpdateKind::Morph:
			return stageVertices( ctx, call, &morph.pose, keepsHistory, "a morphed position is not finite (weights and deltas are finite, their sum with the rest pose overflows; found on the device)",
			                      uploadWeights,
			                      [&]() {
				                      hipLaunchKernelGGL( ptr::morphVertices, grid, group, 0, ctx->stream, morph.pose.dRest, morph.dVertexRun, morph.dVertexEntries, morph.dWeights,
				                                          morph.pose.dStaged, morph.pose.dFlag, (int) V );
			                      } );

		case UpdateKind::Pose:
			return stageVertices( ctx, call, &morph.pose, keepsHistory, "a posed position is not finite (weights, deltas and matrices are finite, the skin of the morphed rest pose overflows; found on the device)",
			                      [&]() {
				                      const hipError_t err = uploadWeights();
				                      return ( err != hipSuccess ) ? err : uploadBones();
			                      },
			                      [&]() {
				                      hipLaunchKernelGGL( ptr::poseVertices, grid, group, 0, ctx->stream, morph.pose.dRest, morph.dVertexRun, morph.dVertexEntries, morph.dWeights,
				                                          skin.dOfVertex, skin.dBones, morph.pose.dStaged, morph.pose.dFlag, (int) V );
			                      } );

		case UpdateKind::SkinDQ:
			return stageVertices( ctx, call, &skin.pose, keepsHistory, "a skinned position is not finite (the dual quaternions are finite, their blend or its product with the rest pose is not; found on the device)",
			                      uploadDualQuats,
			                      [&]() { hipLaunchKernelGGL( ptr::skinVerticesDQ, grid, group, 0, ctx->stream, skin.pose.dRest, skin.dOfVertex, skin.dBones, skin.pose.dStaged, skin.pose.dFlag, (int) V ); } );

		case UpdateKind::PoseDQ:
			return stageVertices( ctx, call, &morph.pose, keepsHistory, "a posed position is not finite (weights, deltas and dual quaternions are finite, the dq skin of the morphed rest pose is not; found on the device)",
			                      [&]() {
				                      const hipError_t err = uploadWeights();
				                      return ( err != hipSuccess ) ? err : uploadDualQuats();
			                      },
			                      [&]() {
				                      hipLaunchKernelGGL( ptr::poseVerticesDQ, grid, group, 0, ctx->stream, morph.pose.dRest, morph.dVertexRun, morph.dVertexEntries, morph.dWeights,
				                                          skin.dOfVertex, skin.dBones, morph.pose.dStaged, morph.pose.dFlag, (int) V );
			                      } );

		default:
			return fail( ctx, PBR_EINVAL, "%s: not a kind that is computed on the device", call );
	}
}

// N' behind the staged V', between evXfNormalsStart and evXfNormalsStop: the one kernel the plan names, from its kind's rest
// normals into the context's.  Nothing when nothing moves the normals.
int launchNormals( pbr_ctx* ctx, NormalKernel which ) {
	if( which == NormalKernel::None ) {
		return PBR_OK;
	}

	const uint32_t N = ctx->scene.numNormals;
	const dim3 grid( ( N + 255 ) / 256 ), group( 256 );
	const SkinState& skin = ctx->scene.skin;
	const MorphState& morph = ctx->scene.morph;
	HIP_TRY( ctx, hipEventRecord( ctx->evXfNormalsStart, ctx->stream ) );

	switch( which ) {
		case NormalKernel::Transform:
			hipLaunchKernelGGL( ptr::transformNormals, grid, group, 0, ctx->stream, ctx->scene.parts.pose.dRestNormals, ctx->scene.parts.dOfNormal, ctx->scene.parts.dRecords,
			                    ctx->scene.dPatchNormals, (int) N );
			break;

		case NormalKernel::Skin:
			hipLaunchKernelGGL( ptr::skinNormals, grid, group, 0, ctx->stream, skin.pose.dRestNormals, skin.dOfNormal, skin.dBones, ctx->scene.dPatchNormals, (int) N );
			break;

		case NormalKernel::Morph:
			hipLaunchKernelGGL( ptr::morphNormals, grid, group, 0, ctx->stream, morph.pose.dRestNormals, morph.dNormalRun, morph.dNormalEntries, morph.dWeights,
			                    ctx->scene.dPatchNormals, (int) N );
			break;

		case NormalKernel::SkinDQ:
			hipLaunchKernelGGL( ptr::skinNormalsDQ, grid, group, 0, ctx->stream, skin.pose.dRestNormals, skin.dOfNormal, skin.dBones, ctx->scene.dPatchNormals, (int) N );
			break;

		case NormalKernel::PoseDQ:
			hipLaunchKernelGGL( ptr::poseNormalsDQ, grid, group, 0, ctx->stream, morph.pose.dRestNormals, morph.dNormalRun, morph.dNormalEntries, morph.dWeights,
			                    skin.dOfNormal, skin.dBones, ctx->scene.dPatchNormals, (int) N );
			break;

		default:
			hipLaunchKernelGGL( ptr::poseNormals, grid, group, 0, ctx->stream, morph.pose.dRestNormals, morph.dNormalRun, morph.dNormalEntries, morph.dWeights,
			                    skin.dOfNormal, skin.dBones, ctx->scene.dPatchNormals, (int) N );
			break;
	}

	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipEventRecord( ctx->evXfNormalsStop, ctx->stream ) );
	return PBR_OK;
}

// The launches every update shares, behind V' and N' in the context's buffers: the face records, the stored face normals, the
// patches (and under Phong tessellation the faces' thick boxes for the leaf step one launch later), the subtrees, the top of
// the tree, and the re-link of the configured layout's records.
int refitBehind( pbr_ctx* ctx, bool gathers, float alpha, bool relinks ) {
	const uint32_t F = ctx->scene.numFaces;
	hipLaunchKernelGGL( ptr::refitFaces, dim3( ( F + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, ctx->scene.dFacesV, ctx->scene.dVertices, ctx->scene.dTris, (int) F );
	HIP_TRY( ctx, hipGetLastError() );

	if( ctx->scene.dFaceN != nullptr ) {
		DevParams P;
		std::memset( &P, 0, sizeof( P ) );
		P.tris = ctx->scene.dTris;
		hipLaunchKernelGGL( ptk::prepareFaceNormals, dim3( ( F + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, P, ctx->scene.dFaceN, (int) F );
		HIP_TRY( ctx, hipGetLastError() );
	}

	if( gathers ) {
		const auto kernel = ( alpha > 0.0f ) ? ptr::refitPatches<true> : ptr::refitPatches<false>;
		hipLaunchKernelGGL( kernel, dim3( ( F + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, ctx->scene.dFacesV, ctx->scene.dPatchFacesN, ctx->scene.dVertices,
		                    ctx->scene.dPatchNormals, ctx->scene.dTriPN, ctx->scene.dFaceBoxes, alpha, (int) F );
		HIP_TRY( ctx, hipGetLastError() );
	}

	const auto subtrees = ( alpha > 0.0f ) ? ptr::refitSubtrees<true> : ptr::refitSubtrees<false>;
	hipLaunchKernelGGL( subtrees, dim3( ctx->scene.refitGroups ), dim3( REFIT_SUBTREE ), 0, ctx->stream, ctx->scene.dRefitSlots, ctx->scene.dRefitInfo,
	                    ctx->scene.dRefitHeights, ctx->scene.dRefitRecordOf, ctx->scene.dFacesV, ctx->scene.dVertices, ctx->scene.dFaceBoxes, ctx->scene.dNodes, ctx->scene.dRootBox );
	HIP_TRY( ctx, hipGetLastError() );

	if( ctx->scene.refitLevels > 0 ) {
		hipLaunchKernelGGL( ptr::refitTop, dim3( 1 ), dim3( REFIT_TOP_THREADS ), 0, ctx->stream, ctx->scene.dRefitTop, ctx->scene.dRefitLevelFirst, (int) ctx->scene.refitLevels,
		                    ctx->scene.dRefitInfo, ctx->scene.dRefitRecordOf, ctx->scene.dNodes, ctx->scene.dRootBox );
		HIP_TRY( ctx, hipGetLastError() );
	}

	ctx->lastRelinked = false;
	ctx->lastRelinkMs = 0.0;
	ctx->lastRelinkLaunches = 0;

	if( relinks ) {
		PBR_TRY( launchRelink( ctx ) );
	}

	return PBR_OK;
}

// Every update call: the refusals (pt_update_host.hpp's two stages around the kind's argument check), the tables a plan needs,
// the step that brings V' and N' to the device, the shared launches, the state.
int updateScene( pbr_ctx* ctx, const UpdateCall& u ) {
	const UpdateKind kind = u.kind;
	const char* call = updateCall( kind );
	const UpdateFacts facts = updateFacts( ctx );
	PBR_TRY( admitKind( kind, facts, &ctx->error ) );
	PBR_TRY( checkUpdateArguments( ctx, u, call ) );
	PBR_TRY( admitShared( kind, u.normals != nullptr, facts, &ctx->error ) );
	const UpdatePlan plan = planUpdate( kind, facts );

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );

	if( plan.gathers ) {
		PBR_TRY( ensurePatchTables( ctx ) );
	}
	if( plan.relinks ) {
		PBR_TRY( ensureRelinkTables( ctx ) );   // its tables first: a call that cannot have them changes nothing
	}

	RestPose* pose = restPoseOf( ctx, kind );

	if( pose != nullptr ) {
		PBR_TRY( stageKind( ctx, kind, call, plan.keepsHistory ) );
		PBR_TRY( launchNormals( ctx, plan.normals ) );
	}
	else {
		// pbr_denoise_temporal: static geometry only — unless motion is tracked: then the history stays, and the first update
		// after a temporal call keeps the positions the history was made under.  The copy runs on the stream, the upload below
		// does not: it waits for the copy
		ctx->temporal.update();

		if( plan.keepsHistory ) {
			PBR_TRY( keepHistoryVertices( ctx, call ) );
		}

		const auto uploadStart = std::chrono::steady_clock::now();
		HIP_TRY( ctx, hipMemcpy( ctx->scene.dVertices, u.vertices, sizeof( pbr_float4 ) * u.num_vertices, hipMemcpyHostToDevice ) );

		if( plan.gathers && u.normals != nullptr ) {
			HIP_TRY( ctx, hipMemcpy( ctx->scene.dPatchNormals, u.normals, sizeof( pbr_float4 ) * u.num_normals, hipMemcpyHostToDevice ) );
		}

		ctx->lastRefitUploadMs = std::chrono::duration<double, std::milli>( std::chrono::steady_clock::now() - uploadStart ).count();
		HIP_TRY( ctx, hipEventRecord( ctx->evStart, ctx->stream ) );
	}

	ctx->geometryGeneration++;   // the context's vertices are new ones from here on: a rest pose captured before is another geometry's
	PBR_TRY( refitBehind( ctx, plan.gathers, plan.alpha, plan.relinks ) );
	HIP_TRY( ctx, hipEventRecord( ctx->evStop, ctx->stream ) );
	PBR_TRY( timedTail( ctx ) );
	ctx->scene.treeStale = true;
	ctx->scene.refitUpdates++;
	ctx->lastUpdate = kind;
	ctx->scene.patchAlpha = plan.alpha;
	ctx->scene.geometryUpdates += updateWasGeometry( kind ) ? 1u : 0u;

	if( pose != nullptr ) {
		float ms = 0.0f, normalsMs = 0.0f;
		HIP_TRY( ctx, hipEventElapsedTime( &ms, ctx->evXfStart, ctx->evXfStop ) );

		if( plan.normals != NormalKernel::None ) {
			HIP_TRY( ctx, hipEventElapsedTime( &normalsMs, ctx->evXfNormalsStart, ctx->evXfNormalsStop ) );
		}

		if( updateDualQuatCode( kind ) != 0 ) {
			// another kind to pbr_diag_skin_info and pbr_diag_morph_info: pbr_diag_skin_dq_info counts these
			ctx->scene.skin.dqLastMs = (double) ms + (double) normalsMs;
			ctx->scene.skin.dqUpdates++;
		}
		else {
			pose->lastMs = (double) ms + (double) normalsMs;
			pose->updates++;
		}
	}

	if( plan.relinks ) {
		// the eight first references are the context's too (applyWalk): 32 bytes of header, no node, box or record
		float ms = 0.0f;
		HIP_TRY( ctx, hipEventElapsedTime( &ms, ctx->evRelinkStart, ctx->evRelinkStop ) );
		HIP_TRY( ctx, hipMemcpy( ctx->scene.walk.walkFirst, ctx->scene.walk.dNodesWalk, sizeof( ctx->scene.walk.walkFirst ), hipMemcpyDeviceToHost ) );
		ctx->lastRelinkMs = (double) ms;
		ctx->lastRelinked = true;
		return PBR_OK;
	}

	freeWalkStreams( ctx );   // none while traversal 0 is configured; an unconfigured context may hold a previous mode's
	// the flag is on but the configured layout's records are not there to re-link: they are built on the host, as pbr_configure does
	return plan.ordered ? buildWalkStreams( ctx, ctx->cfg.traversal ) : PBR_OK;
}

// "Everything new first" of a pbr_set_*: the rest pose's buffers — the normals' only if the call moves them —, the staging
// buffer, the flag word and its pinned twin, and the capture of the context's vertices and normals, device to device (the
// caller's hipDeviceSynchronize waits for it).  On failure *pose is an empty record; the context is not touched either way.
hipError_t allocRestPose( const pbr_ctx* ctx, bool withNormals, RestPose* pose ) {
	const size_t V = ctx->scene.numVertices, N = withNormals ? ctx->scene.numNormals : 0;
	RestPose fresh;
	hipError_t err = (hipError_t) allocAll( { want( fresh.dRest, V ), want( fresh.dStaged, V ), want( fresh.dFlag, 1 ), want( fresh.hFlag, 1 ) } );
	err = ( err != hipSuccess || !withNormals ) ? err : (hipError_t) fresh.dRestNormals.alloc( N );
	err = ( err != hipSuccess ) ? err : hipMemcpy( fresh.dRest, ctx->scene.dVertices, fresh.dRest.bytes(), hipMemcpyDeviceToDevice );
	err = ( err != hipSuccess || !withNormals ) ? err : hipMemcpy( fresh.dRestNormals, ctx->scene.dPatchNormals, fresh.dRestNormals.bytes(), hipMemcpyDeviceToDevice );

	if( err != hipSuccess ) {
		*pose = RestPose();
		return err;
	}

	fresh.normals = withNormals;
	fresh.generation = ctx->geometryGeneration;
	*pose = std::move( fresh );
	return hipSuccess;
}

}  // namespace

int pbr_update_vertices( pbr_ctx* ctx, const pbr_float4* vertices, uint32_t num_vertices ) {
	if( ctx == nullptr || ctx->stream == nullptr ) {
		return fail( ctx, PBR_ESTATE, "context is not usable" );   // a null context too: this call's answer since it exists
	}

	return updateScene( ctx, { UpdateKind::Vertices, vertices, num_vertices, nullptr, 0, nullptr, 0, nullptr, 0 } );
}

int pbr_update_geometry( pbr_ctx* ctx, const pbr_float4* vertices, uint32_t num_vertices, const pbr_float4* normals, uint32_t num_normals ) {
	PBR_TRY( usable( ctx ) );
	return updateScene( ctx, { UpdateKind::Geometry, vertices, num_vertices, normals, num_normals, nullptr, 0, nullptr, 0 } );
}

int pbr_update_transforms( pbr_ctx* ctx, const float* matrices, uint32_t num_parts ) {
	PBR_TRY( usable( ctx ) );
	return updateScene( ctx, { UpdateKind::Transforms, nullptr, 0, nullptr, 0, nullptr, 0, matrices, num_parts } );
}

int pbr_update_skin( pbr_ctx* ctx, const float* matrices, uint32_t num_bones ) {
	PBR_TRY( usable( ctx ) );
	return updateScene( ctx, { UpdateKind::Skin, nullptr, 0, nullptr, 0, nullptr, 0, matrices, num_bones } );
}

int pbr_update_morph( pbr_ctx* ctx, const float* weights, uint32_t num_targets ) {
	PBR_TRY( usable( ctx ) );
	return updateScene( ctx, { UpdateKind::Morph, nullptr, 0, nullptr, 0, weights, num_targets, nullptr, 0 } );
}

int pbr_update_pose( pbr_ctx* ctx, const float* weights, uint32_t num_targets, const float* matrices, uint32_t num_bones ) {
	PBR_TRY( usable( ctx ) );
	return updateScene( ctx, { UpdateKind::Pose, nullptr, 0, nullptr, 0, weights, num_targets, matrices, num_bones } );
}

int pbr_update_skin_dq( pbr_ctx* ctx, const float* dual_quats, uint32_t num_bones ) {
	PBR_TRY( usable( ctx ) );
	return updateScene( ctx, { UpdateKind::SkinDQ, nullptr, 0, nullptr, 0, nullptr, 0, dual_quats, num_bones } );
}

int pbr_update_pose_dq( pbr_ctx* ctx, const float* weights, uint32_t num_targets, const float* dual_quats, uint32_t num_bones ) {
	PBR_TRY( usable( ctx ) );
	return updateScene( ctx, { UpdateKind::PoseDQ, nullptr, 0, nullptr, 0, weights, num_targets, dual_quats, num_bones } );
}

int pbr_dual_quats_from_matrices( const float* matrices, uint32_t num_bones, float* dual_quats_out, char* message, size_t capacity ) {
	std::string why;
	const int status = dualQuatsFromMatrices( matrices, num_bones, dual_quats_out, &why );

	if( message != nullptr && capacity > 0 ) {
		std::snprintf( message, capacity, "%s", why.c_str() );
	}

	return status;
}

int pbr_set_parts( pbr_ctx* ctx, const uint32_t* vertex_part, uint32_t num_vertices, const uint32_t* normal_part, uint32_t num_normals, uint32_t num_parts ) {
	PBR_TRY( usable( ctx ) );

	if( !ctx->hasScene ) {
		return fail( ctx, PBR_ESTATE, "pbr_set_parts before pbr_upload_scene" );
	}

	PBR_TRY( checkParts( vertex_part, num_vertices, ctx->scene.numVertices, normal_part, num_normals, ctx->scene.numNormals, num_parts, &ctx->error ) );

	if( normal_part != nullptr && ctx->scene.dTriPN == nullptr ) {
		return fail( ctx, PBR_ESTATE, "pbr_set_parts: normal parts for a scene that was uploaded without usable vertex normals (its facesN / normals were missing or out of range, it has no Phong patches)" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );

	if( num_parts == 0 ) {
		ctx->scene.parts = PartsState();
		return PBR_OK;
	}
	if( ctx->scene.dTriPN != nullptr ) {
		PBR_TRY( ensurePatchTables( ctx ) );   // a transform gathers the patches again: its tables are made here, not by an update
	}

	// everything new first: a call that cannot have its buffers leaves the parts that were set
	const size_t V = num_vertices, N = num_normals, quad = sizeof( pbr_float4 ), word = sizeof( uint32_t );
	PartsState fresh;
	hipError_t err = allocRestPose( ctx, normal_part != nullptr, &fresh.pose );
	err = ( err != hipSuccess ) ? err : (hipError_t) allocAll( { want( fresh.dOfVertex, V ), want( fresh.dRecords, 6 * (size_t) num_parts ), want( fresh.hRecords, num_parts ) } );
	err = ( err != hipSuccess ) ? err : hipMemcpy( fresh.dOfVertex, vertex_part, word * V, hipMemcpyHostToDevice );

	if( normal_part != nullptr ) {
		err = ( err != hipSuccess ) ? err : (hipError_t) fresh.dOfNormal.alloc( N );
		err = ( err != hipSuccess ) ? err : hipMemcpy( fresh.dOfNormal, normal_part, word * N, hipMemcpyHostToDevice );
	}

	err = ( err != hipSuccess ) ? err : hipDeviceSynchronize();

	if( err != hipSuccess ) {
		return fail( ctx, PBR_EDEVICE, "pbr_set_parts: the rest pose and the part tables: %s", hipGetErrorString( err ) );
	}

	fresh.count = num_parts;
	fresh.pose.bytes = ( quad + quad + word ) * V + ( fresh.pose.normals ? ( quad + word ) * N : 0 ) + sizeof( ptx::PartRecord ) * num_parts + sizeof( unsigned );
	ctx->scene.parts = std::move( fresh );
	return PBR_OK;
}

int pbr_set_skin( pbr_ctx* ctx, const uint32_t* vertex_bones, const float* vertex_weights, uint32_t num_vertices, const uint32_t* normal_bones,
                  const float* normal_weights, uint32_t num_normals, uint32_t num_bones ) {
	PBR_TRY( usable( ctx ) );

	if( !ctx->hasScene ) {
		return fail( ctx, PBR_ESTATE, "pbr_set_skin before pbr_upload_scene" );
	}

	PBR_TRY( checkSkin( vertex_bones, vertex_weights, num_vertices, ctx->scene.numVertices, normal_bones, normal_weights, num_normals, ctx->scene.numNormals, num_bones, &ctx->error ) );

	if( normal_bones != nullptr && ctx->scene.dTriPN == nullptr ) {
		return fail( ctx, PBR_ESTATE, "pbr_set_skin: normal influences for a scene that was uploaded without usable vertex normals (its facesN / normals were missing or out of range, it has no Phong patches)" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );

	if( num_bones == 0 ) {
		ctx->scene.skin = SkinState();
		return PBR_OK;
	}
	if( ctx->scene.dTriPN != nullptr ) {
		PBR_TRY( ensurePatchTables( ctx ) );   // a skin update gathers the patches again: its tables are made here, not by an update
	}

	// the caller's arrays as one 32-byte record per element
	const size_t V = num_vertices, N = num_normals, quad = sizeof( pbr_float4 ), record = sizeof( pts::Influence ), bone = 3 * quad;
	std::vector<pts::Influence> packed( std::max<size_t>( V, N ) );

	// everything new first: a call that cannot have its buffers leaves the skin that was set
	SkinState fresh;
	hipError_t err = allocRestPose( ctx, normal_bones != nullptr, &fresh.pose );
	err = ( err != hipSuccess ) ? err : (hipError_t) allocAll( { want( fresh.dOfVertex, 2 * V ), want( fresh.dBones, 3 * (size_t) num_bones ), want( fresh.hBones, 3 * (size_t) num_bones ) } );
	packInfluences( vertex_bones, vertex_weights, num_vertices, packed.data() );
	err = ( err != hipSuccess ) ? err : hipMemcpy( fresh.dOfVertex, packed.data(), record * V, hipMemcpyHostToDevice );

	if( normal_bones != nullptr ) {
		err = ( err != hipSuccess ) ? err : (hipError_t) fresh.dOfNormal.alloc( 2 * N );
		packInfluences( normal_bones, normal_weights, num_normals, packed.data() );
		err = ( err != hipSuccess ) ? err : hipMemcpy( fresh.dOfNormal, packed.data(), record * N, hipMemcpyHostToDevice );
	}

	err = ( err != hipSuccess ) ? err : hipDeviceSynchronize();

	if( err != hipSuccess ) {
		return fail( ctx, PBR_EDEVICE, "pbr_set_skin: the rest pose and the influence tables: %s", hipGetErrorString( err ) );
	}

	fresh.count = num_bones;
	fresh.pose.bytes = ( quad + quad + record ) * V + ( fresh.pose.normals ? ( quad + record ) * N : 0 ) + bone * num_bones + sizeof( unsigned );
	ctx->scene.skin = std::move( fresh );
	return PBR_OK;
}

int pbr_diag_skin_info( pbr_ctx* ctx, uint64_t out[4], double* ms ) {
	if( ctx == nullptr || out == nullptr ) {
		return fail( ctx, PBR_EINVAL, "pbr_diag_skin_info: null argument" );
	}

	out[0] = ctx->scene.skin.count;
	out[1] = ctx->scene.skin.pose.bytes;
	out[2] = ctx->scene.skin.pose.updates;
	out[3] = ( ctx->lastUpdate == UpdateKind::Skin ) ? 1 : 0;

	if( ms != nullptr ) {
		*ms = ctx->scene.skin.pose.lastMs;
	}

	return PBR_OK;
}

int pbr_diag_skin_dq_info( pbr_ctx* ctx, uint64_t out[2], double* ms ) {
	if( ctx == nullptr || out == nullptr ) {
		return fail( ctx, PBR_EINVAL, "pbr_diag_skin_dq_info: null argument" );
	}

	out[0] = ctx->scene.skin.dqUpdates;
	out[1] = updateDualQuatCode( ctx->lastUpdate );

	if( ms != nullptr ) {
		*ms = ctx->scene.skin.dqLastMs;
	}

	return PBR_OK;
}

int pbr_set_morph( pbr_ctx* ctx, const uint32_t* vertex_first, const uint32_t* vertex_index, const pbr_float4* vertex_delta, const uint32_t* normal_first,
                   const uint32_t* normal_index, const pbr_float4* normal_delta, uint32_t num_targets ) {
	PBR_TRY( usable( ctx ) );

	if( !ctx->hasScene ) {
		return fail( ctx, PBR_ESTATE, "pbr_set_morph before pbr_upload_scene" );
	}

	PBR_TRY( checkMorph( vertex_first, vertex_index, vertex_delta, normal_first, normal_index, normal_delta, num_targets, ctx->scene.numVertices, ctx->scene.numNormals, &ctx->error ) );

	if( normal_first != nullptr && ctx->scene.dTriPN == nullptr ) {
		return fail( ctx, PBR_ESTATE, "pbr_set_morph: normal targets for a scene that was uploaded without usable vertex normals (its facesN / normals were missing or out of range, it has no Phong patches)" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );

	if( num_targets == 0 ) {
		ctx->scene.morph = MorphState();
		return PBR_OK;
	}

	// the caller's target-major lists as element-major runs
	const bool withNormals = ( normal_first != nullptr );
	const size_t V = ctx->scene.numVertices, N = withNormals ? ctx->scene.numNormals : 0, T = num_targets, quad = sizeof( pbr_float4 ), word = sizeof( uint32_t );
	const size_t Ev = vertex_first[T], En = withNormals ? normal_first[T] : 0;
	std::vector<uint32_t> vertexRun( V + 1 ), normalRun( withNormals ? N + 1 : 0 );
	std::vector<ptm::Entry> vertexEntries( Ev ), normalEntries( En );
	PBR_TRY( packMorph( vertex_first, vertex_index, vertex_delta, num_targets, (uint32_t) V, vertexRun.data(), vertexEntries.data(), &ctx->error ) );

	if( withNormals ) {
		PBR_TRY( packMorph( normal_first, normal_index, normal_delta, num_targets, (uint32_t) N, normalRun.data(), normalEntries.data(), &ctx->error ) );
	}
	if( ctx->scene.dTriPN != nullptr ) {
		PBR_TRY( ensurePatchTables( ctx ) );   // a morph update gathers the patches again: its tables are made here, not by an update
	}

	// everything new first: a call that cannot have its buffers leaves the morph that was set
	MorphState fresh;
	hipError_t err = allocRestPose( ctx, withNormals, &fresh.pose );
	err = ( err != hipSuccess ) ? err : (hipError_t) allocAll( { want( fresh.dVertexRun, V + 1 ), want( fresh.dVertexEntries, Ev ), want( fresh.dWeights, T ), want( fresh.hWeights, T ) } );
	err = ( err != hipSuccess ) ? err : hipMemcpy( fresh.dVertexRun, vertexRun.data(), word * ( V + 1 ), hipMemcpyHostToDevice );
	err = ( err != hipSuccess || Ev == 0 ) ? err : hipMemcpy( fresh.dVertexEntries, vertexEntries.data(), quad * Ev, hipMemcpyHostToDevice );

	if( withNormals ) {
		err = ( err != hipSuccess ) ? err : (hipError_t) allocAll( { want( fresh.dNormalRun, N + 1 ), want( fresh.dNormalEntries, En ) } );
		err = ( err != hipSuccess ) ? err : hipMemcpy( fresh.dNormalRun, normalRun.data(), word * ( N + 1 ), hipMemcpyHostToDevice );
		err = ( err != hipSuccess || En == 0 ) ? err : hipMemcpy( fresh.dNormalEntries, normalEntries.data(), quad * En, hipMemcpyHostToDevice );
	}

	err = ( err != hipSuccess ) ? err : hipDeviceSynchronize();

	if( err != hipSuccess ) {
		return fail( ctx, PBR_EDEVICE, "pbr_set_morph: the rest pose and the target tables: %s", hipGetErrorString( err ) );
	}

	fresh.count = num_targets;
	fresh.vertexEntries = Ev;
	fresh.normalEntries = En;
	fresh.pose.bytes = quad * V + quad * V + word * ( V + 1 ) + quad * Ev + ( withNormals ? quad * N + word * ( N + 1 ) + quad * En : 0 ) + sizeof( float ) * T + sizeof( unsigned );
	ctx->scene.morph = std::move( fresh );
	return PBR_OK;
}

int pbr_diag_morph_info( pbr_ctx* ctx, uint64_t out[6], double* ms ) {
	if( ctx == nullptr || out == nullptr ) {
		return fail( ctx, PBR_EINVAL, "pbr_diag_morph_info: null argument" );
	}

	out[0] = ctx->scene.morph.count;
	out[1] = ctx->scene.morph.vertexEntries;
	out[2] = ctx->scene.morph.normalEntries;
	out[3] = ctx->scene.morph.pose.bytes;
	out[4] = ctx->scene.morph.pose.updates;
	out[5] = updateMorphCode( ctx->lastUpdate );

	if( ms != nullptr ) {
		*ms = ctx->scene.morph.pose.lastMs;
	}

	return PBR_OK;
}

int pbr_read_geometry( pbr_ctx* ctx, pbr_float4* vertices_out, uint32_t vcap, uint32_t* num_vertices, pbr_float4* normals_out, uint32_t ncap, uint32_t* num_normals ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}
	if( !ctx->hasScene ) {
		return fail( ctx, PBR_ESTATE, "pbr_read_geometry before pbr_upload_scene" );
	}
	if( num_vertices == nullptr || num_normals == nullptr ) {
		return fail( ctx, PBR_EINVAL, "pbr_read_geometry: null num_vertices or num_normals" );
	}

	*num_vertices = ctx->scene.numVertices;
	*num_normals = ( ctx->scene.dTriPN != nullptr ) ? ctx->scene.numNormals : 0;   // normals nobody can use were not kept

	if( vertices_out != nullptr && vcap < *num_vertices ) {
		return fail( ctx, PBR_EINVAL, "pbr_read_geometry: room for %u vertices, the scene has %u", vcap, *num_vertices );
	}
	if( normals_out != nullptr && ncap < *num_normals ) {
		return fail( ctx, PBR_EINVAL, "pbr_read_geometry: room for %u normals, the scene has %u", ncap, *num_normals );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );

	if( vertices_out != nullptr && *num_vertices > 0 ) {
		HIP_TRY( ctx, hipMemcpy( vertices_out, ctx->scene.dVertices, sizeof( pbr_float4 ) * *num_vertices, hipMemcpyDeviceToHost ) );
	}
	if( normals_out != nullptr && *num_normals > 0 ) {
		if( ctx->scene.dPatchNormals != nullptr ) {
			HIP_TRY( ctx, hipMemcpy( normals_out, ctx->scene.dPatchNormals, sizeof( pbr_float4 ) * *num_normals, hipMemcpyDeviceToHost ) );
		}
		else {
			std::memcpy( normals_out, ctx->scene.patchNormals.data(), sizeof( pbr_float4 ) * *num_normals );   // still the upload's host copy
		}
	}

	return PBR_OK;
}

int pbr_diag_transform_info( pbr_ctx* ctx, uint64_t out[4], double* ms ) {
	if( ctx == nullptr || out == nullptr ) {
		return fail( ctx, PBR_EINVAL, "pbr_diag_transform_info: null argument" );
	}

	out[0] = ctx->scene.parts.count;
	out[1] = ctx->scene.parts.pose.bytes;
	out[2] = ctx->scene.parts.pose.updates;
	out[3] = ( ctx->lastUpdate == UpdateKind::Transforms ) ? 1 : 0;

	if( ms != nullptr ) {
		*ms = ctx->scene.parts.pose.lastMs;
	}

	return PBR_OK;
}

int pbr_read_bvh( pbr_ctx* ctx, pbr_bvh_node* nodes_out, uint32_t capacity, uint32_t* num_nodes ) {
	if( ctx == nullptr || !ctx->hasScene ) {
		return fail( ctx, PBR_ESTATE, "pbr_read_bvh before pbr_upload_scene" );
	}
	if( num_nodes == nullptr ) {
		return fail( ctx, PBR_EINVAL, "pbr_read_bvh: null num_nodes" );
	}

	*num_nodes = ctx->scene.tree.size();

	if( nodes_out == nullptr ) {
		return PBR_OK;
	}
	if( capacity < ctx->scene.tree.size() ) {
		return fail( ctx, PBR_EINVAL, "pbr_read_bvh: room for %u nodes, the tree has %u", capacity, ctx->scene.tree.size() );
	}

	PBR_TRY( refreshTree( ctx ) );
	std::memcpy( nodes_out, ctx->scene.tree.bvh.data(), sizeof( pbr_bvh_node ) * ctx->scene.tree.size() );
	return PBR_OK;
}

int pbr_configure( pbr_ctx* ctx, const pbr_config* cfg ) {
	if( ctx == nullptr || ctx->stream == nullptr ) {
		return fail( ctx, PBR_ESTATE, "context is not usable" );
	}
	if( cfg == nullptr ) {
		return fail( ctx, PBR_EINVAL, "configure: null config" );
	}
	if( cfg->width == 0 || cfg->height == 0 || ( cfg->width & 7u ) || ( cfg->height & 7u ) ) {
		return fail( ctx, PBR_EINVAL, "width / height must be non-zero multiples of 8 (opencl.localgroupsize, config.json:85)" );
	}
	if( cfg->brdf > 1 || cfg->shadow_rays > 1 ) {
		return fail( ctx, PBR_EINVAL, "brdf and shadow_rays must be 0 or 1" );
	}
	if( cfg->max_depth == 0 || cfg->samples == 0 ) {
		return fail( ctx, PBR_EINVAL, "max_depth and samples must be >= 1" );
	}
	if( cfg->phong_tessellation > 0.0f && ctx->hasScene && ctx->scene.dTriPN == nullptr ) {
		return fail( ctx, PBR_EINVAL, "Phong tessellation needs vertex normals: the uploaded scene's facesN / normals are missing or out of range" );
	}
	if( cfg->phong_tessellation > 0.0f && ctx->hasScene && ctx->scene.refitUpdates > 0 && !updateWasGeometry( ctx->lastUpdate ) ) {
		return fail( ctx, PBR_ESTATE, "Phong tessellation after pbr_update_vertices: the refitted boxes are tight boxes of the flat triangles and would clip the patches, and the patches' corners were not updated — upload the scene again, or call pbr_update_geometry under this phong_tessellation" );
	}
	if( cfg->phong_tessellation > 0.0f && ctx->hasScene && ctx->scene.refitUpdates > 0 && !( ctx->scene.patchAlpha == cfg->phong_tessellation ) ) {
		return fail( ctx, PBR_ESTATE, "Phong tessellation %g after a pbr_update_geometry under %g: the boxes were thickened for that value and could clip these patches — configure %g, or upload the scene again", (double) cfg->phong_tessellation, (double) ctx->scene.patchAlpha, (double) ctx->scene.patchAlpha );
	}
	if( cfg->traversal > 3 || cfg->arith > 1 ) {
		return fail( ctx, PBR_EINVAL, "traversal must be 0 (the reference's walk), 1 (six orders), 2 (eight orders) or 3 (eight orders, compact records); arith 0 (exact) or 1 (native)" );
	}
	if( cfg->tile_world == 0 || cfg->tile_rank >= cfg->tile_world ) {
		return fail( ctx, PBR_EINVAL, "tile_rank must be < tile_world, tile_world >= 1" );
	}

	// the records of the configured walk for the scene there is, unless they are there already: packed before anything changes
	PackedWalk walk;
	const bool packsWalk = ( ctx->hasScene && ctx->scene.walk.walkBuilt != cfg->traversal );

	if( packsWalk && cfg->traversal != 0 ) {
		PBR_TRY( refreshTree( ctx ) );   // after pbr_update_vertices: the orders are built from the refitted boxes
	}

	PBR_TRY( packConfiguredWalk( ctx, *cfg, packsWalk ? &ctx->scene.tree : nullptr, &walk ) );

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	freeImages( ctx );

	ctx->cfg = *cfg;
	ctx->tilesX = (int) ( cfg->width / 8 );
	ctx->tilesY = (int) ( cfg->height / 8 );
	ctx->numTiles = ctx->tilesX * ctx->tilesY;
	// tiles t = j * world + rank, j = 0 .. : count those below numTiles
	ctx->numLocalTiles = ( ctx->numTiles - (int) cfg->tile_rank + (int) cfg->tile_world - 1 ) / (int) cfg->tile_world;

	// Every context can hold the full image (import_tiles scatters all ranks' tiles into imgOut).
	const size_t fullBytes = sizeof( float4 ) * 64 * (size_t) ctx->numTiles;
	Images& I = ctx->images;
	const size_t fullSlots = 64 * (size_t) ctx->numTiles;
	HIP_TRY( ctx, allocAll( { want( I.dImgIn, fullSlots ), want( I.dImgOut, fullSlots ), want( I.dImgDbg, fullSlots ), want( I.dRows, fullSlots ) } ) );
	HIP_TRY( ctx, hipMemset( ctx->images.dImgIn, 0, fullBytes ) );
	HIP_TRY( ctx, hipMemset( ctx->images.dImgOut, 0, fullBytes ) );
	HIP_TRY( ctx, hipMemset( ctx->images.dImgDbg, 0, fullBytes ) );
	HIP_TRY( ctx, hipMemset( ctx->dCounters, 0, sizeof( unsigned long long ) * kCounterSlots ) );
	HIP_TRY( ctx, hipDeviceSynchronize() );   // the memsets ran on the null stream; launches use ctx->stream

	// the local tiles as a grid for the banded queue: its true shape when unsharded, about that when sharded
	ctx->queueGrid = dealGrid( ctx->tilesX, ctx->numLocalTiles, (int) cfg->tile_world );
	spatialTileOrder( ctx->queueGrid, ctx->numLocalTiles, PT_BANDS, &ctx->images.deal[kDealSpatial].host, ctx->images.deal[kDealSpatial].first );
	const size_t tiles = ctx->images.deal[kDealSpatial].host.size();

	for( int order = 0; order < kDealOrders; order++ ) {
		// a context without local tiles gets no table of the first two orders (a null pointer: learnTileCosts then learns nothing)
		const size_t entries = ( order == kDealExpensiveLast ) ? std::max<size_t>( 1, tiles ) : tiles;

		if( entries > 0 ) {
			HIP_TRY( ctx, I.deal[order].dev.alloc( entries ) );
		}
	}

	HIP_TRY( ctx, I.dTileCost.alloc( std::max<size_t>( 1, tiles ) ) );
	ctx->costLearnt = false;
	ctx->launchesSinceLearn = 0;
	PBR_TRY( uploadTileOrder( ctx ) );
	replan( ctx );   // a new scene / configuration is tuned afresh
	ctx->configured = true;

	if( !walk.storage.empty() ) {
		return uploadWalkStreams( ctx, walk, cfg->traversal );
	}
	if( ctx->scene.walk.walkBuilt != cfg->traversal ) {
		freeWalkStreams( ctx );   // the records of a traversal that is no longer configured
	}

	return PBR_OK;
}

int pbr_write_input( pbr_ctx* ctx, const float* rgba ) {
	if( ctx == nullptr || !ctx->configured ) {
		return fail( ctx, PBR_ESTATE, "write_input before pbr_configure" );
	}
	if( rgba == nullptr ) {
		return fail( ctx, PBR_EINVAL, "write_input: null source" );
	}

	ctx->varianceCurrent = false;
	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	HIP_TRY( ctx, hipMemcpyAsync( ctx->images.dRows, rgba, sizeof( float4 ) * ctx->cfg.width * ctx->cfg.height, hipMemcpyHostToDevice, ctx->stream ) );
	const size_t n = (size_t) ctx->numLocalTiles * 64;
	hipLaunchKernelGGL( ptk::retile, dim3( (unsigned) ( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, ctx->stream,
		ctx->images.dRows, ctx->images.dImgIn, (int) ctx->cfg.width, ctx->numLocalTiles, ctx->tilesX, (int) ctx->cfg.tile_world, (int) ctx->cfg.tile_rank );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	return PBR_OK;
}

int pbr_reset_accum( pbr_ctx* ctx ) {
	if( ctx == nullptr || !ctx->configured ) {
		return fail( ctx, PBR_ESTATE, "reset_accum before pbr_configure" );
	}

	ctx->varianceCurrent = false;
	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	const size_t fullBytes = sizeof( float4 ) * 64 * (size_t) ctx->numTiles;
	HIP_TRY( ctx, hipMemsetAsync( ctx->images.dImgIn, 0, fullBytes, ctx->stream ) );
	HIP_TRY( ctx, hipMemsetAsync( ctx->dCounters, 0, sizeof( unsigned long long ) * kCounterSlots, ctx->stream ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	return PBR_OK;
}

int pbr_render_frame( pbr_ctx* ctx, float seed, float pixelWeight, float pxDim, const pbr_camera* cam ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}

	return launch( ctx, 0, 1, &seed, true, pixelWeight, pxDim, cam );
}

int pbr_accumulate( pbr_ctx* ctx ) {
	if( ctx == nullptr || !ctx->configured ) {
		return fail( ctx, PBR_ESTATE, "accumulate before pbr_configure" );
	}

	ctx->varianceCurrent = false;
	ctx->images.dImgIn.swap( ctx->images.dImgOut );
	return PBR_OK;
}

int pbr_render( pbr_ctx* ctx, uint32_t first_sample_count, uint32_t n_frames, const float* seeds, float pxDim, const pbr_camera* cam ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}
	if( cam != nullptr && cam->focusPoint[0] >= 0 && cam->focusPoint[1] >= 0 ) {
		return fail( ctx, PBR_EINVAL, "pbr_render needs focusPoint < 0; with depth of field call pbr_render_frame + pbr_accumulate per frame" );
	}

	PBR_TRY( launch( ctx, first_sample_count, n_frames, seeds, false, 0.0f, pxDim, cam ) );

	// result in imageOut AND imageIn
	const size_t bytes = sizeof( float4 ) * 64 * (size_t) ctx->numLocalTiles;
	HIP_TRY( ctx, hipMemcpyAsync( ctx->images.dImgIn, ctx->images.dImgOut, bytes, hipMemcpyDeviceToDevice, ctx->stream ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	return PBR_OK;
}

int pbr_render_dof( pbr_ctx* ctx, uint32_t first_sample_count, uint32_t n_frames, const float* seeds, float pxDim, const pbr_camera* cam ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}

	PBR_TRY( launch( ctx, first_sample_count, n_frames, seeds, false, 0.0f, pxDim, cam, true ) );

	// result in imageOut AND imageIn
	const size_t bytes = sizeof( float4 ) * 64 * (size_t) ctx->numLocalTiles;
	HIP_TRY( ctx, hipMemcpyAsync( ctx->images.dImgIn, ctx->images.dImgOut, bytes, hipMemcpyDeviceToDevice, ctx->stream ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	return PBR_OK;
}

int pbr_render_adaptive( pbr_ctx* ctx, uint32_t first_sample_count, const float* seeds, float pxDim, const pbr_camera* cam, const pbr_adaptive_params* params ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}

	std::string why;

	if( adaptiveCheck( params, seeds, cam, &why ) != PBR_OK ) {
		return fail( ctx, PBR_EINVAL, "%s", why.c_str() );
	}

	PBR_TRY( launchAdaptive( ctx, first_sample_count, seeds, pxDim, cam, *params ) );

	// result in imageOut AND imageIn, as pbr_render leaves it
	const size_t bytes = sizeof( float4 ) * 64 * (size_t) ctx->numLocalTiles;
	HIP_TRY( ctx, hipMemcpyAsync( ctx->images.dImgIn, ctx->images.dImgOut, bytes, hipMemcpyDeviceToDevice, ctx->stream ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	ctx->varianceFirstCount = first_sample_count;
	ctx->varianceCurrent = true;   // the moments and the frame counts are those of the image as it stands
	ctx->temporalFresh = true;     // pbr_denoise_temporal: a render it has not integrated yet
	return PBR_OK;
}

int pbr_read_tile_stats( pbr_ctx* ctx, uint32_t* frames, float* error, uint32_t capacity, uint32_t* count ) {
	if( ctx == nullptr || count == nullptr ) {
		return fail( ctx, PBR_EINVAL, "read_tile_stats: null argument" );
	}
	if( !ctx->configured || !ctx->adaptiveStats ) {
		return fail( ctx, PBR_ESTATE, "read_tile_stats before pbr_render_adaptive" );
	}

	*count = (uint32_t) ctx->numLocalTiles;

	if( frames == nullptr && error == nullptr ) {
		return PBR_OK;
	}
	if( capacity < *count ) {
		return fail( ctx, PBR_EINVAL, "read_tile_stats: %u entries for %u local tiles", capacity, *count );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );

	if( frames != nullptr ) {
		HIP_TRY( ctx, hipMemcpyAsync( frames, ctx->images.dTileFrames, sizeof( uint32_t ) * *count, hipMemcpyDeviceToHost, ctx->stream ) );
	}
	if( error != nullptr ) {
		HIP_TRY( ctx, hipMemcpyAsync( error, ctx->images.dTileError, sizeof( float ) * *count, hipMemcpyDeviceToHost, ctx->stream ) );
	}

	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	return PBR_OK;
}

int pbr_read_output( pbr_ctx* ctx, float* rgba ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}
	return readTiled( ctx, ctx->images.dImgOut, rgba, (int) ctx->cfg.tile_world, (int) ctx->cfg.tile_rank );
}

int pbr_get_focus_depth( pbr_ctx* ctx, int x, int y, float* t, int* owned ) {
	if( ctx == nullptr || t == nullptr || owned == nullptr ) {
		return fail( ctx, PBR_EINVAL, "get_focus_depth: null argument" );
	}
	if( !ctx->configured ) {
		return fail( ctx, PBR_ESTATE, "get_focus_depth before pbr_configure" );
	}

	// CLAMP_TO_EDGE, as the sampler of getPreviousFocus has it (pathtracing.cl:58-65)
	const int fx = std::max( 0, std::min( (int) ctx->cfg.width - 1, x ) );
	const int fy = std::max( 0, std::min( (int) ctx->cfg.height - 1, y ) );
	const int tile = ( fy >> 3 ) * ctx->tilesX + ( fx >> 3 );
	*t = 0.0f;
	const int position = ptk::dealPositionOfTile( tile, ctx->tilesX, (int) ctx->cfg.tile_world );
	*owned = ( position % (int) ctx->cfg.tile_world == (int) ctx->cfg.tile_rank ) ? 1 : 0;

	if( *owned ) {
		const size_t slot = (size_t) ( position / (int) ctx->cfg.tile_world ) * 64 + (size_t) ( ( fy & 7 ) * 8 + ( fx & 7 ) );
		float4 pixel;
		HIP_TRY( ctx, hipSetDevice( ctx->device ) );
		HIP_TRY( ctx, hipMemcpyAsync( &pixel, ctx->images.dImgIn + slot, sizeof( pixel ), hipMemcpyDeviceToHost, ctx->stream ) );
		HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
		*t = pixel.w;
	}

	return PBR_OK;
}

int pbr_set_focus_depth( pbr_ctx* ctx, float t ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}

	ctx->focusGiven = true;
	ctx->focusDepth = t;
	return PBR_OK;
}

int pbr_read_display( pbr_ctx* ctx, uint8_t* rgba8, int top_row_first ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}
	if( !ctx->configured ) {
		return fail( ctx, PBR_ESTATE, "read before pbr_configure" );
	}
	if( rgba8 == nullptr ) {
		return fail( ctx, PBR_EINVAL, "read: null destination" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	// dRows (16 B per pixel) doubles as the 4-B-per-pixel staging buffer
	hipLaunchKernelGGL( ptk::displayRGBA8, imageGrid( (int) ctx->cfg.width, (int) ctx->cfg.height ), kImageBlock, 0, ctx->stream, (const float4*) ctx->images.dImgOut, (uchar4*) ctx->images.dRows.get(),
		(int) ctx->cfg.width, (int) ctx->cfg.height, ctx->tilesX, (int) ctx->cfg.tile_world, (int) ctx->cfg.tile_rank, top_row_first ? 1 : 0 );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipMemcpyAsync( rgba8, ctx->images.dRows, (size_t) 4 * ctx->cfg.width * ctx->cfg.height, hipMemcpyDeviceToHost, ctx->stream ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	return PBR_OK;
}

// ---- pbr_display: exposure, tone curve and transfer function on the device (pt_display_host.hpp, pt_display.hpp) ----

namespace {

// merge rounds of the histogram kernel without the "display_merge" knob: DESIGN.md 5.5e has the measurement
const int kDisplayMerge = 2;

void launchDisplayHistogram( pbr_ctx* ctx, const float4* pixels, size_t groups ) {
	const dim3 grid( ptv::histogramBlocks( groups ) ), block( ptv::kHistogramBlock );
	unsigned* counts = ctx->images.dDisplayCounts;
	const int knob = ctx->knobs.displayMerge;

	switch( ( knob == 0 || knob == 1 || knob == 2 || knob == 4 ) ? knob : kDisplayMerge ) {
		case 0: hipLaunchKernelGGL( ptv::displayHistogram<0>, grid, block, 0, ctx->stream, pixels, (unsigned) groups, counts ); break;
		case 1: hipLaunchKernelGGL( ptv::displayHistogram<1>, grid, block, 0, ctx->stream, pixels, (unsigned) groups, counts ); break;
		case 4: hipLaunchKernelGGL( ptv::displayHistogram<4>, grid, block, 0, ctx->stream, pixels, (unsigned) groups, counts ); break;
		default: hipLaunchKernelGGL( ptv::displayHistogram<2>, grid, block, 0, ctx->stream, pixels, (unsigned) groups, counts ); break;
	}
}

// The counters, their pinned twin and the table: all of them or none, and the table uploaded — or none of them.
int displayBuffers( pbr_ctx* ctx ) {
	Images& I = ctx->images;

	if( !I.dDisplayCounts.empty() ) {
		return PBR_OK;
	}

	HIP_TRY( ctx, allocAll( { want( I.dDisplayCounts, (size_t) ptv::kCountSlots ), want( I.hDisplayCounts, (size_t) ptv::kCountSlots ), want( I.dDisplayTable, (size_t) 256 ) } ) );
	const hipError_t err = hipMemcpy( I.dDisplayTable, ptv::kSrgbThreshold, sizeof( ptv::kSrgbThreshold ), hipMemcpyHostToDevice );

	if( err != hipSuccess ) {
		I.dDisplayCounts.reset();
		I.hDisplayCounts.reset();
		I.dDisplayTable.reset();
		return fail( ctx, PBR_EDEVICE, "pbr_display: uploading the sRGB table: %s", hipGetErrorString( err ) );
	}

	return PBR_OK;
}

}  // namespace

int pbr_display( pbr_ctx* ctx, const pbr_display_params* params, const float* rgba, uint8_t* rgba8, int top_row_first, pbr_display_info* info ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}
	if( ctx->stream == nullptr ) {
		return fail( ctx, PBR_ESTATE, "context is not usable" );
	}
	if( !ctx->configured ) {
		return fail( ctx, PBR_ESTATE, "pbr_display before pbr_configure" );
	}
	if( rgba8 == nullptr ) {
		return fail( ctx, PBR_EINVAL, "pbr_display: null destination" );
	}

	std::string why;
	const int admitted = checkDisplayParams( params, &why );

	if( admitted != PBR_OK ) {
		return fail( ctx, admitted, "%s", why.c_str() );
	}

	const bool automatic = ( params->exposure_mode == PBR_DISPLAY_EXPOSURE_AUTO );
	const bool sharded = ( ctx->cfg.tile_world > 1 );

	if( automatic && rgba == nullptr && sharded ) {
		return fail( ctx, PBR_ESTATE, "pbr_display: auto exposure over a shard's tiles (tile_world %u): its histogram is not the image's — gather the frame (pbr_import_tiles, pbr_read_full) and pass it as rgba", ctx->cfg.tile_world );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	PBR_TRY( displayBuffers( ctx ) );
	Images& I = ctx->images;
	const size_t pixels = (size_t) ctx->cfg.width * ctx->cfg.height;
	const float4* source = I.dImgOut;
	size_t groups = (size_t) ctx->numLocalTiles;

	if( rgba != nullptr ) {
		HIP_TRY( ctx, I.dDisplaySource.grow( pixels ) );
		HIP_TRY( ctx, hipMemcpyAsync( I.dDisplaySource, rgba, sizeof( float4 ) * pixels, hipMemcpyHostToDevice, ctx->stream ) );
		source = I.dDisplaySource;
		groups = pixels / 64;   // width and height are multiples of 8
	}

	const bool counts = automatic || info != nullptr;
	const uint32_t* n = I.hDisplayCounts;

	if( counts ) {
		HIP_TRY( ctx, hipMemsetAsync( I.dDisplayCounts, 0, sizeof( unsigned ) * ptv::kCountSlots, ctx->stream ) );
		HIP_TRY( ctx, hipEventRecord( ctx->evHistogramStart, ctx->stream ) );
		launchDisplayHistogram( ctx, source, groups );
		HIP_TRY( ctx, hipGetLastError() );
		HIP_TRY( ctx, hipEventRecord( ctx->evHistogramStop, ctx->stream ) );
		HIP_TRY( ctx, hipMemcpyAsync( I.hDisplayCounts, I.dDisplayCounts, sizeof( unsigned ) * ptv::kCountSlots, hipMemcpyDeviceToHost, ctx->stream ) );
	}

	// auto: the host reads the counts between the two kernels
	float exposure = params->exposure;
	double target = 0.0, used = 0.0;
	uint64_t counted = 0;

	if( automatic ) {
		HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
		target = displayTarget( n, *params, ctx->displayAdapted, ctx->displayLog2, &counted );
		used = displayAdapt( target, *params, ctx->displayAdapted, ctx->displayLog2 );
		exposure = displayExposure( *params, used );
	}

	ptv::MapArgs A;
	A.exposure = exposure;
	A.white = params->white;
	A.curve = params->curve;
	A.transfer = params->transfer;
	A.width = (int) ctx->cfg.width;
	A.height = (int) ctx->cfg.height;
	A.rowMajor = ( rgba != nullptr ) ? 1 : 0;
	A.tilesX = ctx->tilesX;
	A.tileWorld = (int) ctx->cfg.tile_world;
	A.tileRank = (int) ctx->cfg.tile_rank;
	A.topRowFirst = top_row_first ? 1 : 0;
	HIP_TRY( ctx, hipEventRecord( ctx->evStart, ctx->stream ) );
	// dRows (16 B per pixel) doubles as the 4-B-per-pixel staging buffer, as in pbr_read_display
	hipLaunchKernelGGL( ptv::displayMap, imageGrid( A.width, A.height ), kImageBlock, 0, ctx->stream, source, (const float*) I.dDisplayTable, (uchar4*) I.dRows.get(), A );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipEventRecord( ctx->evStop, ctx->stream ) );
	HIP_TRY( ctx, hipMemcpyAsync( rgba8, I.dRows, 4 * pixels, hipMemcpyDeviceToHost, ctx->stream ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	float histogramMs = 0.0f, mapMs = 0.0f;

	if( counts ) {
		HIP_TRY( ctx, hipEventElapsedTime( &histogramMs, ctx->evHistogramStart, ctx->evHistogramStop ) );
	}

	HIP_TRY( ctx, hipEventElapsedTime( &mapMs, ctx->evStart, ctx->evStop ) );
	ctx->lastHistogramMs = (double) histogramMs;
	ctx->lastMapMs = (double) mapMs;
	ctx->lastKernelMs = (double) histogramMs + (double) mapMs;

	if( info != nullptr ) {
		counted = 0;

		for( int b = 0; b < ptv::kBins; b++ ) {
			info->histogram[b] = n[b];
			counted += n[b];
		}

		info->exposure = exposure;
		info->log2_target = target;
		info->log2_used = used;
		info->counted = counted;
		// the tiles of other ranks read 0, as the map sees them
		info->dark = (uint64_t) n[ptv::kDarkSlot] + ( ( rgba == nullptr ) ? 64u * (uint64_t) ( ctx->numTiles - ctx->numLocalTiles ) : 0u );
	}

	if( automatic ) {
		ctx->displayAdapted = true;
		ctx->displayLog2 = used;
	}

	return PBR_OK;
}

int pbr_display_reset( pbr_ctx* ctx ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}

	ctx->displayAdapted = false;
	return PBR_OK;
}

int pbr_diag_display_info( pbr_ctx* ctx, double* histogram_ms, double* map_ms ) {
	if( ctx == nullptr || histogram_ms == nullptr || map_ms == nullptr ) {
		return fail( ctx, PBR_EINVAL, "pbr_diag_display_info: null argument" );
	}

	*histogram_ms = ctx->lastHistogramMs;
	*map_ms = ctx->lastMapMs;
	return PBR_OK;
}

int pbr_read_debug( pbr_ctx* ctx, float* rgba ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}
	return readTiled( ctx, ctx->images.dImgDbg, rgba, (int) ctx->cfg.tile_world, (int) ctx->cfg.tile_rank );
}

int pbr_get_counters( pbr_ctx* ctx, pbr_counters* out ) {
	if( ctx == nullptr || out == nullptr || ctx->stream == nullptr ) {
		return fail( ctx, PBR_EINVAL, "get_counters: null argument" );
	}

	unsigned long long host[4] = { 0, 0, 0, 0 };
	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	HIP_TRY( ctx, hipMemcpy( host, ctx->dCounters, sizeof( host ), hipMemcpyDeviceToHost ) );
	out->nodes = host[0];
	out->tris = host[1];
	out->hits = host[2];
	out->paths = host[3];
	return PBR_OK;
}

double pbr_last_kernel_ms( const pbr_ctx* ctx ) {
	return ( ctx != nullptr ) ? ctx->lastKernelMs : 0.0;
}

uint64_t pbr_tile_bytes( const pbr_ctx* ctx ) {
	if( ctx == nullptr || !ctx->configured ) {
		return 0;
	}

	const uint64_t perRank = (uint64_t) ( ( ctx->numTiles + (int) ctx->cfg.tile_world - 1 ) / (int) ctx->cfg.tile_world );
	return perRank * 1024u;
}

int pbr_export_tiles( pbr_ctx* ctx, void* d_dst ) {
	if( ctx == nullptr || !ctx->configured ) {
		return fail( ctx, PBR_ESTATE, "export_tiles before pbr_configure" );
	}
	if( d_dst == nullptr ) {
		return fail( ctx, PBR_EINVAL, "export_tiles: null destination" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	const size_t bytes = sizeof( float4 ) * 64 * (size_t) ctx->numLocalTiles;
	HIP_TRY( ctx, hipMemsetAsync( d_dst, 0, (size_t) pbr_tile_bytes( ctx ), ctx->stream ) );
	HIP_TRY( ctx, hipMemcpyAsync( d_dst, ctx->images.dImgOut, bytes, hipMemcpyDeviceToDevice, ctx->stream ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	return PBR_OK;
}

int pbr_import_tiles( pbr_ctx* ctx, const void* d_all ) {
	if( ctx == nullptr || !ctx->configured ) {
		return fail( ctx, PBR_ESTATE, "import_tiles before pbr_configure" );
	}
	if( d_all == nullptr ) {
		return fail( ctx, PBR_EINVAL, "import_tiles: null source" );
	}

	ctx->varianceCurrent = false;
	HIP_TRY( ctx, hipSetDevice( ctx->device ) );

	HIP_TRY( ctx, ctx->images.dFull.grow( 64 * (size_t) ctx->numTiles ) );

	const int perRank = ( ctx->numTiles + (int) ctx->cfg.tile_world - 1 ) / (int) ctx->cfg.tile_world;
	const size_t n = (size_t) ctx->numTiles * 64;
	hipLaunchKernelGGL( ptk::scatterGathered, dim3( (unsigned) ( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, ctx->stream,
		(const float4*) d_all, ctx->images.dFull, ctx->numTiles, perRank, (int) ctx->cfg.tile_world, ctx->tilesX );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	return PBR_OK;
}

int pbr_read_full( pbr_ctx* ctx, float* rgba ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}
	return readTiled( ctx, ctx->images.dFull, rgba, 1, 0 );
}


// ---- the denoise family: pbr_denoise, pbr_read_variance, pbr_denoise_guided, pbr_denoise_temporal ----------------------
// What the calls refuse, the pass schedule and the camera terms are host arithmetic: pt_denoise_host.hpp.

namespace {

// a per-call buffer of bytes: the diagnostics and the builders cast it to what their kernels take
typedef Owned<unsigned char> DevBuf;

// The planes pbr_denoise and pbr_denoise_guided allocate per call: the first-hit features and the filter's two working planes.
struct FilterPlanes {
	Owned<float4> position, normal, albedo, ping, pong;

	int alloc( size_t pixels ) {
		return allocAll( { want( position, pixels ), want( normal, pixels ), want( albedo, pixels ), want( ping, pixels ), want( pong, pixels ) } );
	}
};

// The front of every call of the family: a scene and a configuration first, then what pt_denoise_host.hpp's check of the
// arguments said (status, why) — its message becomes the context's error.
int admit( pbr_ctx* ctx, const char* who, int status = PBR_OK, const std::string& why = std::string() ) {
	if( !ctx->hasScene || !ctx->configured ) {
		return fail( ctx, PBR_ESTATE, "%s before pbr_upload_scene / pbr_configure", who );
	}

	return ( status == PBR_OK ) ? PBR_OK : fail( ctx, status, "%s", why.c_str() );
}

// pbr_read_variance / pbr_denoise_guided / pbr_denoise_temporal: the moments must describe the accumulated image as it is
int varianceUsable( pbr_ctx* ctx, const char* who ) {
	if( ctx->cfg.tile_world > 1 ) {
		return fail( ctx, PBR_ESTATE, "%s with tile sharding: the variance pbr_render_adaptive keeps of other ranks' tiles is not gathered", who );
	}
	if( !ctx->varianceCurrent || ctx->images.dMoments == nullptr ) {
		return fail( ctx, PBR_ESTATE, "%s needs the accumulated image as the last pbr_render_adaptive left it: no adaptive call yet, or the image was written since", who );
	}

	return PBR_OK;
}

// an output the caller may leave out (null): copied behind whatever the stream holds
int readBack( pbr_ctx* ctx, void* dst, const void* src, size_t bytes ) {
	if( dst != nullptr ) {
		HIP_TRY( ctx, hipMemcpyAsync( dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream ) );
	}

	return PBR_OK;
}

// {position, normal, albedo} into the caller's `features` (may be null)
int readFeatures( pbr_ctx* ctx, float* features, const FilterPlanes& D, size_t pixels ) {
	if( features != nullptr ) {
		PBR_TRY( readBack( ctx, features, D.position, sizeof( float4 ) * pixels ) );
		PBR_TRY( readBack( ctx, features + 4 * pixels, D.normal, sizeof( float4 ) * pixels ) );
		PBR_TRY( readBack( ctx, features + 8 * pixels, D.albedo, sizeof( float4 ) * pixels ) );
	}

	return PBR_OK;
}

// `passes` launches of ptd::atrousGuidedPass: the first reads `in` (and leaves it as it is), every pass writes the plane of
// `outs` the one before it did not; the last one restores .w from `original` and writes `varianceOut`.  -> the plane that
// holds the result.  The caller checks hipGetLastError.
const float4* guidedPasses( pbr_ctx* ctx, const pbr_denoise_guided_params& params, int w, int h, float pxDim, const float4* in, float4* const outs[2],
                            const float4* position, const float4* normal, const float4* albedo, const float4* original, float* varianceOut ) {
	for( uint32_t pass = 0; pass < params.passes; pass++ ) {
		const bool last = ( pass + 1 == params.passes );
		float4* const out = outs[pass & 1u];
		hipLaunchKernelGGL( ptd::atrousGuidedPass, imageGrid( w, h ), kImageBlock, 0, ctx->stream, ptd::guidedPass( params, pass, w, h, pxDim ), in, out,
			position, normal, albedo, last ? original : (const float4*) nullptr, last ? varianceOut : (float*) nullptr );
		in = out;
	}

	return in;
}

// `passes` launches of ptd::atrousPass, ping-pong between `in` and `out`: the first reads `in`, the second overwrites it.
// -> the plane that holds the result.  The caller checks hipGetLastError.
const float4* plainPasses( pbr_ctx* ctx, const pbr_denoise_params& params, int w, int h, float pxDim, float4* in, float4* out,
                           const float4* position, const float4* normal, const float4* albedo ) {
	for( uint32_t pass = 0; pass < params.passes; pass++ ) {
		hipLaunchKernelGGL( ptd::atrousPass, imageGrid( w, h ), kImageBlock, 0, ctx->stream, ptd::plainPass( params, pass, w, h, pxDim ), (const float4*) in, out,
			position, normal, albedo );
		std::swap( in, out );
	}

	return in;
}

// Steps 0 to 4 of pbr_denoise_temporal (pt_temporal.hpp) over device planes: temporalMotion in front when `motion`, then
// temporalIntegrate< motion >.  working holds {C, V} and receives I; info may be null.  Without `motion` the planes from
// `face` on are not touched.  The caller checks hipGetLastError.
struct TemporalStepPlanes {
	float4* working;
	const float4* position, * normal, * albedo;
	const float4* prevI, * prevPosition, * prevNormal, * prevAlbedo;
	const unsigned* prevLengths;
	unsigned* lengths;
	float4* info;
	const int* face;
	const uint4* facesV;
	const float4* vertices, * histVertices;
	float4* motion, * reference;
};

void temporalSteps( pbr_ctx* ctx, const ptd::TemporalArgs& A, int w, int h, bool motion, const TemporalStepPlanes& S ) {
	const dim3 grid = imageGrid( w, h );

	if( motion ) {
		hipLaunchKernelGGL( ptd::temporalMotion, grid, kImageBlock, 0, ctx->stream, w, h, S.face, S.position, S.normal,
			S.facesV, S.vertices, S.histVertices, S.motion, S.reference );
	}

	const auto integrate = motion ? ptd::temporalIntegrate<true> : ptd::temporalIntegrate<false>;
	hipLaunchKernelGGL( integrate, grid, kImageBlock, 0, ctx->stream, A, S.working, S.position, S.normal, S.albedo,
		S.prevI, S.prevPosition, S.prevNormal, S.prevAlbedo, S.prevLengths, S.lengths, S.info,
		(const float4*) ( motion ? S.motion : nullptr ), (const float4*) ( motion ? S.reference : nullptr ) );
}

}  // namespace

// The denoise half of the display step (csrc/pt_denoise.hpp): first-hit features from one primary ray per pixel, then
// edge-avoiding a-trous passes over the accumulated image.  Leaves the accumulation untouched.
int pbr_denoise( pbr_ctx* ctx, float pxDim, const pbr_camera* cam, const pbr_denoise_params* params, float* rgba, float* features ) {
	if( ctx == nullptr || ctx->stream == nullptr ) {
		return PBR_EINVAL;
	}

	std::string why;
	PBR_TRY( admit( ctx, "pbr_denoise", ptd::denoiseCheck( "pbr_denoise", cam, params, rgba, &why ), why ) );
	const bool sharded = ctx->cfg.tile_world > 1;

	if( sharded && ctx->images.dFull == nullptr ) {
		return fail( ctx, PBR_ESTATE, "pbr_denoise with tile sharding filters the gathered frame: call pbr_import_tiles first" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	const int w = (int) ctx->cfg.width, h = (int) ctx->cfg.height;
	const size_t pixels = (size_t) w * (size_t) h;
	FilterPlanes D;
	HIP_TRY( ctx, D.alloc( pixels ) );

	DevParams P;
	PBR_TRY( sceneParams( ctx, &P ) );
	setCamera( &P, cam, w, h, pxDim );

	const dim3 grid = imageGrid( w, h );
	HIP_TRY( ctx, hipEventRecord( ctx->evStart, ctx->stream ) );
	hipLaunchKernelGGL( ptk::untile, grid, kImageBlock, 0, ctx->stream, (const float4*) ( sharded ? ctx->images.dFull : ctx->images.dImgOut ), (float4*) D.ping,
		w, h, ctx->tilesX, 1, 0 );
	hipLaunchKernelGGL( ptd::firstHitFeatures, grid, kImageBlock, 0, ctx->stream, P, (float4*) D.position, (float4*) D.normal, (float4*) D.albedo, (int*) nullptr );
	HIP_TRY( ctx, hipGetLastError() );

	const float4* result = plainPasses( ctx, *params, w, h, pxDim, (float4*) D.ping, (float4*) D.pong, (const float4*) D.position,
		(const float4*) D.normal, (const float4*) D.albedo );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipEventRecord( ctx->evStop, ctx->stream ) );
	PBR_TRY( readBack( ctx, rgba, result, sizeof( float4 ) * pixels ) );
	PBR_TRY( readFeatures( ctx, features, D, pixels ) );
	return timedTail( ctx );
}

// The variance of every pixel's mean luminance after pbr_render_adaptive (csrc/pt_denoise_guided.hpp, pixelVariance).
int pbr_read_variance( pbr_ctx* ctx, float* variance ) {
	if( ctx == nullptr || ctx->stream == nullptr ) {
		return PBR_EINVAL;
	}
	if( variance == nullptr ) {
		return fail( ctx, PBR_EINVAL, "pbr_read_variance: null destination" );
	}

	PBR_TRY( admit( ctx, "pbr_read_variance" ) );
	PBR_TRY( varianceUsable( ctx, "pbr_read_variance" ) );
	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	const int w = (int) ctx->cfg.width, h = (int) ctx->cfg.height;
	HIP_TRY( ctx, hipEventRecord( ctx->evStart, ctx->stream ) );
	// dRows (W x H float4) is the staging of every read-back: its first quarter holds the floats
	hipLaunchKernelGGL( ptd::pixelVariance, imageGrid( w, h ), kImageBlock, 0, ctx->stream, (const float2*) ctx->images.dMoments, (const unsigned*) ctx->images.dTileFrames,
		ctx->varianceFirstCount, (const float4*) nullptr, (float*) ctx->images.dRows.get(), (float4*) nullptr, w, h, ctx->tilesX );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipEventRecord( ctx->evStop, ctx->stream ) );
	HIP_TRY( ctx, hipMemcpyAsync( variance, ctx->images.dRows, sizeof( float ) * (size_t) w * (size_t) h, hipMemcpyDeviceToHost, ctx->stream ) );
	return timedTail( ctx );
}

// pbr_denoise with the adaptive render's variance in place of sigma_color (csrc/pt_denoise_guided.hpp): the luminance term is
// in units of the local standard deviation, and the variance is filtered along.  Leaves the accumulation, the moments and
// the tile stats untouched.
int pbr_denoise_guided( pbr_ctx* ctx, float pxDim, const pbr_camera* cam, const pbr_denoise_guided_params* params,
                        float* rgba, float* variance_out, float* features ) {
	if( ctx == nullptr || ctx->stream == nullptr ) {
		return PBR_EINVAL;
	}

	std::string why;
	PBR_TRY( admit( ctx, "pbr_denoise_guided", ptd::denoiseCheck( "pbr_denoise_guided", cam, params, rgba, &why ), why ) );
	PBR_TRY( varianceUsable( ctx, "pbr_denoise_guided" ) );
	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	const int w = (int) ctx->cfg.width, h = (int) ctx->cfg.height;
	const size_t pixels = (size_t) w * (size_t) h;
	FilterPlanes D;
	DevBuf dOriginal, dVariance;
	HIP_TRY( ctx, D.alloc( pixels ) );
	HIP_TRY( ctx, dOriginal.alloc( sizeof( float4 ) * pixels ) );
	HIP_TRY( ctx, dVariance.alloc( sizeof( float ) * pixels ) );

	DevParams P;
	PBR_TRY( sceneParams( ctx, &P ) );
	setCamera( &P, cam, w, h, pxDim );

	const dim3 grid = imageGrid( w, h );
	HIP_TRY( ctx, hipEventRecord( ctx->evStart, ctx->stream ) );
	hipLaunchKernelGGL( ptk::untile, grid, kImageBlock, 0, ctx->stream, (const float4*) ctx->images.dImgOut, (float4*) dOriginal.get(), w, h, ctx->tilesX, 1, 0 );
	hipLaunchKernelGGL( ptd::pixelVariance, grid, kImageBlock, 0, ctx->stream, (const float2*) ctx->images.dMoments, (const unsigned*) ctx->images.dTileFrames,
		ctx->varianceFirstCount, (const float4*) dOriginal.get(), (float*) nullptr, (float4*) D.ping, w, h, ctx->tilesX );
	hipLaunchKernelGGL( ptd::firstHitFeatures, grid, kImageBlock, 0, ctx->stream, P, (float4*) D.position, (float4*) D.normal, (float4*) D.albedo, (int*) nullptr );
	HIP_TRY( ctx, hipGetLastError() );

	float4* const outs[2] = { (float4*) D.pong, (float4*) D.ping };
	const float4* result = guidedPasses( ctx, *params, w, h, pxDim, (const float4*) D.ping, outs, (const float4*) D.position, (const float4*) D.normal,
		(const float4*) D.albedo, (const float4*) dOriginal.get(), (float*) dVariance.get() );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipEventRecord( ctx->evStop, ctx->stream ) );
	PBR_TRY( readBack( ctx, rgba, result, sizeof( float4 ) * pixels ) );
	PBR_TRY( readBack( ctx, variance_out, dVariance.get(), sizeof( float ) * pixels ) );
	PBR_TRY( readFeatures( ctx, features, D, pixels ) );
	return timedTail( ctx );
}

// The filters of pbr_denoise (kind 0) and pbr_denoise_guided / pbr_denoise_temporal (kind 1) over planes the caller supplies
// (include/pbr_hip_diag.h): the public calls' pass drivers, grid, block and ping-pong, with nothing of the context but its
// device and stream.
int pbr_diag_filter( pbr_ctx* ctx, int kind, int width, int height, float pxDim, const void* params, const float* image, const float* variance,
                     const float* features, float* rgba_out, float* variance_out ) {
	if( ctx == nullptr || ctx->stream == nullptr ) {
		return PBR_EINVAL;
	}
	if( kind < 0 || kind > 1 || params == nullptr || image == nullptr || features == nullptr || rgba_out == nullptr || ( kind == 1 && variance == nullptr ) ) {
		return fail( ctx, PBR_EINVAL, "pbr_diag_filter: kind 0 / 1, and no null parameters, image, features, destination or (kind 1) variance" );
	}
	if( width < 1 || height < 1 || (uint64_t) width * (uint64_t) height > ( 1ull << 20 ) ) {
		return fail( ctx, PBR_EINVAL, "pbr_diag_filter: width, height >= 1 and width * height <= 1 Mi (got %d x %d)", width, height );
	}

	const pbr_denoise_params* plain = ( kind == 0 ) ? (const pbr_denoise_params*) params : nullptr;
	const pbr_denoise_guided_params* guided = ( kind == 1 ) ? (const pbr_denoise_guided_params*) params : nullptr;
	std::string why;
	const int status = ( kind == 0 ) ? ptd::filterCheck( "pbr_diag_filter", *plain, &why ) : ptd::filterCheck( "pbr_diag_filter", *guided, &why );

	if( status != PBR_OK ) {
		return fail( ctx, status, "%s", why.c_str() );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	const size_t pixels = (size_t) width * (size_t) height;
	FilterPlanes D;
	DevBuf dOriginal, dVariance;
	HIP_TRY( ctx, D.alloc( pixels ) );
	HIP_TRY( ctx, hipMemcpyAsync( D.position, features, sizeof( float4 ) * pixels, hipMemcpyHostToDevice, ctx->stream ) );
	HIP_TRY( ctx, hipMemcpyAsync( D.normal, features + 4 * pixels, sizeof( float4 ) * pixels, hipMemcpyHostToDevice, ctx->stream ) );
	HIP_TRY( ctx, hipMemcpyAsync( D.albedo, features + 8 * pixels, sizeof( float4 ) * pixels, hipMemcpyHostToDevice, ctx->stream ) );
	const float4* result = nullptr;
	std::vector<float> working;

	if( kind == 0 ) {
		HIP_TRY( ctx, hipMemcpyAsync( D.ping, image, sizeof( float4 ) * pixels, hipMemcpyHostToDevice, ctx->stream ) );
		result = plainPasses( ctx, *plain, width, height, pxDim, (float4*) D.ping, (float4*) D.pong, (const float4*) D.position,
			(const float4*) D.normal, (const float4*) D.albedo );
	} else {
		// the filter's first input as pixelVariance builds `working`: {r, g, b, var}
		working.assign( image, image + 4 * pixels );

		for( size_t at = 0; at < pixels; at++ ) {
			working[4 * at + 3] = variance[at];
		}

		HIP_TRY( ctx, dOriginal.alloc( sizeof( float4 ) * pixels ) );
		HIP_TRY( ctx, dVariance.alloc( sizeof( float ) * pixels ) );
		HIP_TRY( ctx, hipMemcpyAsync( dOriginal.get(), image, sizeof( float4 ) * pixels, hipMemcpyHostToDevice, ctx->stream ) );
		HIP_TRY( ctx, hipMemcpyAsync( D.ping, working.data(), sizeof( float4 ) * pixels, hipMemcpyHostToDevice, ctx->stream ) );
		float4* const outs[2] = { (float4*) D.pong, (float4*) D.ping };
		result = guidedPasses( ctx, *guided, width, height, pxDim, (const float4*) D.ping, outs, (const float4*) D.position,
			(const float4*) D.normal, (const float4*) D.albedo, (const float4*) dOriginal.get(), (float*) dVariance.get() );
	}

	HIP_TRY( ctx, hipGetLastError() );
	// staged, so that a call that fails on the device has written nothing
	std::vector<float> rgba( 4 * pixels ), var( ( kind == 1 && variance_out != nullptr ) ? pixels : 0 );
	PBR_TRY( readBack( ctx, rgba.data(), result, sizeof( float4 ) * pixels ) );
	PBR_TRY( readBack( ctx, var.empty() ? nullptr : var.data(), dVariance.get(), sizeof( float ) * pixels ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	std::copy( rgba.begin(), rgba.end(), rgba_out );
	std::copy( var.begin(), var.end(), variance_out );
	return PBR_OK;
}

// Steps 0 to 4 of pbr_denoise_temporal over planes the caller supplies (include/pbr_hip_diag.h): the public call's driver, grid,
// block and by-value arguments, with nothing of the context but its device and stream.
int pbr_diag_temporal( pbr_ctx* ctx, int width, int height, float pxDim, const pbr_camera* cam, const pbr_temporal_params* temporal,
                       const float* image, const float* variance, const float* features,
                       const float* prev_integrated, const float* prev_features, const uint32_t* prev_lengths, const pbr_camera* prev_cam, float prev_pxDim,
                       const int32_t* face, const uint32_t* facesV, uint32_t num_faces, const float* vertices, const float* hist_vertices, uint32_t num_vertices,
                       float* integrated, float* history, uint32_t* lengths, float* motion, float* reference ) {
	if( ctx == nullptr || ctx->stream == nullptr ) {
		return PBR_EINVAL;
	}
	if( cam == nullptr || temporal == nullptr || image == nullptr || variance == nullptr || features == nullptr || integrated == nullptr
	        || history == nullptr || lengths == nullptr ) {
		return fail( ctx, PBR_EINVAL, "pbr_diag_temporal: no null camera, parameters, image, variance, features, integrated, history or lengths" );
	}
	if( width < 1 || height < 1 || (uint64_t) width * (uint64_t) height > ( 1ull << 20 ) ) {
		return fail( ctx, PBR_EINVAL, "pbr_diag_temporal: width, height >= 1 and width * height <= 1 Mi (got %d x %d)", width, height );
	}

	std::string why;
	const int status = ptd::temporalCheck( "pbr_diag_temporal", *temporal, &why );

	if( status != PBR_OK ) {
		return fail( ctx, status, "%s", why.c_str() );
	}

	const int prevGiven = ( prev_integrated != nullptr ) + ( prev_features != nullptr ) + ( prev_lengths != nullptr ) + ( prev_cam != nullptr );
	const int motionGiven = ( face != nullptr ) + ( facesV != nullptr ) + ( vertices != nullptr ) + ( hist_vertices != nullptr );

	if( ( prevGiven != 0 && prevGiven != 4 ) || ( motionGiven != 0 && motionGiven != 4 ) ) {
		return fail( ctx, PBR_EINVAL, "pbr_diag_temporal: the previous state, and the motion inputs, are given whole or not at all" );
	}

	const bool hasHistory = ( prevGiven == 4 ), moving = ( motionGiven == 4 );

	if( moving && !hasHistory ) {
		return fail( ctx, PBR_EINVAL, "pbr_diag_temporal: motion inputs without a previous state" );
	}
	if( moving && ( motion == nullptr || reference == nullptr || num_faces < 1 || num_vertices < 1 || num_faces > ( 1u << 24 ) || num_vertices > ( 1u << 24 ) ) ) {
		return fail( ctx, PBR_EINVAL, "pbr_diag_temporal: the motion path needs motion and reference destinations and 1 .. 16 Mi faces and vertices" );
	}

	const size_t pixels = (size_t) width * (size_t) height;

	// what keeps the kernels' gathers in bounds, and Hl + 1 inside the definition
	if( hasHistory ) {
		for( size_t at = 0; at < pixels; at++ ) {
			if( prev_lengths[at] < 1u || prev_lengths[at] > 1024u ) {
				return fail( ctx, PBR_EINVAL, "pbr_diag_temporal: prev_lengths must be in 1 .. 1024 (pixel %zu: %u)", at, prev_lengths[at] );
			}
		}
	}
	if( moving ) {
		for( size_t at = 0; at < pixels; at++ ) {
			if( face[at] < -1 || (int64_t) face[at] >= (int64_t) num_faces ) {
				return fail( ctx, PBR_EINVAL, "pbr_diag_temporal: face must be in [-1, num_faces) (pixel %zu: %d)", at, face[at] );
			}
		}
		for( size_t f = 0; f < num_faces; f++ ) {
			for( int k = 0; k < 3; k++ ) {
				if( facesV[4 * f + k] >= num_vertices ) {
					return fail( ctx, PBR_EINVAL, "pbr_diag_temporal: facesV corner >= num_vertices (face %zu)", f );
				}
			}
		}
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	const size_t plane = sizeof( float4 ) * pixels;
	DevBuf dWorking, dFeatures, dPrevI, dPrevFeatures, dPrevLengths, dLengths, dInfo, dFace, dFacesV, dVertices, dHistVertices, dMotion, dReference;
	HIP_TRY( ctx, dWorking.alloc( plane ) );
	HIP_TRY( ctx, dFeatures.alloc( 3 * plane ) );
	HIP_TRY( ctx, dLengths.alloc( sizeof( unsigned ) * pixels ) );
	HIP_TRY( ctx, dInfo.alloc( plane ) );
	// the working plane as pixelVariance builds it: {r, g, b, var}
	std::vector<float> working( image, image + 4 * pixels );

	for( size_t at = 0; at < pixels; at++ ) {
		working[4 * at + 3] = variance[at];
	}

	HIP_TRY( ctx, hipMemcpyAsync( dWorking.get(), working.data(), plane, hipMemcpyHostToDevice, ctx->stream ) );
	HIP_TRY( ctx, hipMemcpyAsync( dFeatures.get(), features, 3 * plane, hipMemcpyHostToDevice, ctx->stream ) );

	if( hasHistory ) {
		HIP_TRY( ctx, dPrevI.alloc( plane ) );
		HIP_TRY( ctx, dPrevFeatures.alloc( 3 * plane ) );
		HIP_TRY( ctx, dPrevLengths.alloc( sizeof( unsigned ) * pixels ) );
		HIP_TRY( ctx, hipMemcpyAsync( dPrevI.get(), prev_integrated, plane, hipMemcpyHostToDevice, ctx->stream ) );
		HIP_TRY( ctx, hipMemcpyAsync( dPrevFeatures.get(), prev_features, 3 * plane, hipMemcpyHostToDevice, ctx->stream ) );
		HIP_TRY( ctx, hipMemcpyAsync( dPrevLengths.get(), prev_lengths, sizeof( unsigned ) * pixels, hipMemcpyHostToDevice, ctx->stream ) );
	}
	if( moving ) {
		HIP_TRY( ctx, dFace.alloc( sizeof( int ) * pixels ) );
		HIP_TRY( ctx, dFacesV.alloc( sizeof( uint4 ) * num_faces ) );
		HIP_TRY( ctx, dVertices.alloc( sizeof( float4 ) * num_vertices ) );
		HIP_TRY( ctx, dHistVertices.alloc( sizeof( float4 ) * num_vertices ) );
		HIP_TRY( ctx, dMotion.alloc( plane ) );
		HIP_TRY( ctx, dReference.alloc( plane ) );
		HIP_TRY( ctx, hipMemcpyAsync( dFace.get(), face, sizeof( int ) * pixels, hipMemcpyHostToDevice, ctx->stream ) );
		HIP_TRY( ctx, hipMemcpyAsync( dFacesV.get(), facesV, sizeof( uint4 ) * num_faces, hipMemcpyHostToDevice, ctx->stream ) );
		HIP_TRY( ctx, hipMemcpyAsync( dVertices.get(), vertices, sizeof( float4 ) * num_vertices, hipMemcpyHostToDevice, ctx->stream ) );
		HIP_TRY( ctx, hipMemcpyAsync( dHistVertices.get(), hist_vertices, sizeof( float4 ) * num_vertices, hipMemcpyHostToDevice, ctx->stream ) );
	}

	// without a previous state the old camera is never read by a pixel: this call's stands in
	const ptd::TemporalArgs A = ptd::temporalArgs( *temporal, width, height, pxDim, hasHistory, hasHistory ? *prev_cam : *cam,
		hasHistory ? prev_pxDim : pxDim, ptd::cameraTerms( *cam, width, height, pxDim ) );
	const float4* dF = (const float4*) dFeatures.get();
	const float4* dPF = (const float4*) dPrevFeatures.get();
	const TemporalStepPlanes S = { (float4*) dWorking.get(), dF, dF + pixels, dF + 2 * pixels,
		(const float4*) dPrevI.get(), dPF, hasHistory ? dPF + pixels : nullptr, hasHistory ? dPF + 2 * pixels : nullptr,
		(const unsigned*) dPrevLengths.get(), (unsigned*) dLengths.get(), (float4*) dInfo.get(), (const int*) dFace.get(), (const uint4*) dFacesV.get(),
		(const float4*) dVertices.get(), (const float4*) dHistVertices.get(), (float4*) dMotion.get(), (float4*) dReference.get() };
	temporalSteps( ctx, A, width, height, moving, S );
	HIP_TRY( ctx, hipGetLastError() );
	// staged, so that a call that fails on the device has written nothing
	std::vector<float> outI( 4 * pixels ), outInfo( 4 * pixels ), outMotion( moving ? 4 * pixels : 0 ), outReference( moving ? 4 * pixels : 0 );
	std::vector<uint32_t> outLengths( pixels );
	PBR_TRY( readBack( ctx, outI.data(), dWorking.get(), plane ) );
	PBR_TRY( readBack( ctx, outInfo.data(), dInfo.get(), plane ) );
	PBR_TRY( readBack( ctx, outLengths.data(), dLengths.get(), sizeof( uint32_t ) * pixels ) );
	PBR_TRY( readBack( ctx, moving ? outMotion.data() : nullptr, dMotion.get(), plane ) );
	PBR_TRY( readBack( ctx, moving ? outReference.data() : nullptr, dReference.get(), plane ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	std::copy( outI.begin(), outI.end(), integrated );
	std::copy( outInfo.begin(), outInfo.end(), history );
	std::copy( outLengths.begin(), outLengths.end(), lengths );
	std::copy( outMotion.begin(), outMotion.end(), motion );
	std::copy( outReference.begin(), outReference.end(), reference );
	return PBR_OK;
}

// pbr_denoise_temporal's history is dropped: the next call starts every pixel at L = 1.
int pbr_temporal_reset( pbr_ctx* ctx ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}

	ctx->temporal.drop();
	return PBR_OK;
}

// Per-vertex motion for pbr_denoise_temporal: while it is on, pbr_update_vertices keeps the history (and the vertex positions it
// was made under) instead of dropping it.  A flag of the context: needs no scene, survives pbr_configure and pbr_upload_scene.
int pbr_temporal_track_motion( pbr_ctx* ctx, int on ) {
	PBR_TRY( usable( ctx ) );

	ctx->temporal.track( on != 0 );

	if( on == 0 && ctx->scene.dHistVertices != nullptr ) {
		HIP_TRY( ctx, hipSetDevice( ctx->device ) );
		ctx->scene.dHistVertices.reset();
	}

	return PBR_OK;
}

// The planes of the last successful pbr_denoise_temporal's motion step: {Pprev, code} and the first-hit face per pixel.
int pbr_read_temporal_motion( pbr_ctx* ctx, float* motion, int32_t* face ) {
	PBR_TRY( usable( ctx ) );
	if( !ctx->temporal.lastMotion || ctx->images.planes.face == nullptr ) {
		return fail( ctx, PBR_ESTATE, "pbr_read_temporal_motion: the last successful pbr_denoise_temporal did not take the motion path (it needs pbr_temporal_track_motion, a history and a pbr_update_vertices since that history)" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	const size_t pixels = (size_t) ctx->cfg.width * (size_t) ctx->cfg.height;
	PBR_TRY( readBack( ctx, motion, ctx->images.planes.motion, sizeof( float4 ) * pixels ) );
	PBR_TRY( readBack( ctx, face, ctx->images.planes.face, sizeof( int32_t ) * pixels ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	return PBR_OK;
}

// pbr_denoise_guided with a history in front of the filter (csrc/pt_temporal.hpp): the previous call's integrated colour and
// variance are fetched through the previous camera, blended with this render by sample weight, filtered, and kept — before
// the filter — for the next call.  Leaves the accumulation, the moments and the tile stats untouched.
int pbr_denoise_temporal( pbr_ctx* ctx, float pxDim, const pbr_camera* cam, const pbr_temporal_params* temporal, const pbr_denoise_guided_params* filter,
                          float* rgba, float* variance_out, float* integrated, float* history ) {
	if( ctx == nullptr || ctx->stream == nullptr ) {
		return PBR_EINVAL;
	}

	std::string why;
	PBR_TRY( admit( ctx, "pbr_denoise_temporal", ptd::denoiseTemporalCheck( "pbr_denoise_temporal", cam, temporal, filter, rgba, &why ), why ) );
	PBR_TRY( varianceUsable( ctx, "pbr_denoise_temporal" ) );

	if( !ctx->temporalFresh ) {
		return fail( ctx, PBR_ESTATE, "pbr_denoise_temporal has integrated this render already: it needs a new pbr_render_adaptive before every call" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	const int w = (int) ctx->cfg.width, h = (int) ctx->cfg.height;
	const size_t pixels = (size_t) w * (size_t) h;
	TemporalPlanes& T = ctx->images.planes;
	// static geometry, or per-vertex motion in front of the integration (pt_temporal_host.hpp decides).  The planes come with
	// the first call since pbr_configure, the motion path's with the first call that takes it; new planes are no history
	const TemporalPolicy::Path path = ctx->temporal.path();
	const bool motion = ( path == TemporalPolicy::MOTION ), first = T.variance.empty();

	if( T.alloc( pixels, motion ) != 0 ) {
		return fail( ctx, PBR_EDEVICE, "pbr_denoise_temporal: no device memory for the history" );
	}
	if( first ) {
		ctx->temporal.drop();
	}
	if( motion && ( ctx->scene.dHistVertices == nullptr || ctx->scene.dFacesV == nullptr ) ) {
		return fail( ctx, PBR_ESTATE, "pbr_denoise_temporal: the history's vertex positions are missing" );   // cannot happen: `moved` implies the copy
	}

	const int prev = T.set, cur = 1 - prev;
	float4* dI = T.integrated[cur];
	const float4* dPosition = T.position[cur];
	const float4* dNormal = T.normal[cur];
	const float4* dAlbedo = T.albedo[cur];
	float4* dOriginal = ctx->images.dRows;   // the staging of every read-back: free between calls

	DevParams P;
	PBR_TRY( sceneParams( ctx, &P ) );
	const ptd::TemporalArgs A = ptd::temporalArgs( *temporal, w, h, pxDim, ctx->temporal.history, ctx->temporalCam, ctx->temporalPxDim,
		setCamera( &P, cam, w, h, pxDim ) );

	const dim3 grid = imageGrid( w, h );
	HIP_TRY( ctx, hipEventRecord( ctx->evStart, ctx->stream ) );
	hipLaunchKernelGGL( ptk::untile, grid, kImageBlock, 0, ctx->stream, (const float4*) ctx->images.dImgOut, dOriginal, w, h, ctx->tilesX, 1, 0 );
	hipLaunchKernelGGL( ptd::pixelVariance, grid, kImageBlock, 0, ctx->stream, (const float2*) ctx->images.dMoments, (const unsigned*) ctx->images.dTileFrames,
		ctx->varianceFirstCount, (const float4*) dOriginal, (float*) nullptr, dI, w, h, ctx->tilesX );
	hipLaunchKernelGGL( ptd::firstHitFeatures, grid, kImageBlock, 0, ctx->stream, P, T.position[cur], T.normal[cur], T.albedo[cur], motion ? T.face : (int*) nullptr );

	const TemporalStepPlanes S = { dI, dPosition, dNormal, dAlbedo, T.integrated[prev], T.position[prev], T.normal[prev], T.albedo[prev],
		T.length[prev], T.length[cur], ( history != nullptr ) ? T.info : (float4*) nullptr, T.face, (const uint4*) ctx->scene.dFacesV,
		(const float4*) ctx->scene.dVertices, (const float4*) ctx->scene.dHistVertices, T.motion, T.reference };
	temporalSteps( ctx, A, w, h, motion, S );
	HIP_TRY( ctx, hipGetLastError() );

	// the first pass reads I and leaves it as it is: it is the next call's history
	float4* const outs[2] = { T.ping, T.pong };
	const float4* result = guidedPasses( ctx, *filter, w, h, pxDim, dI, outs, dPosition, dNormal, dAlbedo, dOriginal, T.variance );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipEventRecord( ctx->evStop, ctx->stream ) );
	PBR_TRY( readBack( ctx, rgba, result, sizeof( float4 ) * pixels ) );
	PBR_TRY( readBack( ctx, variance_out, T.variance, sizeof( float ) * pixels ) );
	PBR_TRY( readBack( ctx, integrated, dI, sizeof( float4 ) * pixels ) );
	PBR_TRY( readBack( ctx, history, T.info, sizeof( float4 ) * pixels ) );
	PBR_TRY( timedTail( ctx ) );
	// the set just written becomes the history, by pointer
	T.set = cur;
	ctx->temporal.succeeded( path );   // ... made under the current vertices
	ctx->temporalFresh = false;
	ctx->temporalCam = *cam;
	ctx->temporalPxDim = pxDim;
	return PBR_OK;
}

uint32_t pbr_bvh_node_capacity( uint32_t num_faces ) {
	// every face its own leaf is the most records a binary tree over them can have; at least a container and a leaf
	return ( num_faces < 2 ) ? 2u : 2u * num_faces - 1u;
}

namespace {

// the radix-tree builder of round 1 (Karras 2012), kept for comparison: PBR_BVH_BUILDER=lbvh
int buildRadixTree( pbr_ctx* ctx, ptb::BuildArrays B, uint32_t num_faces, uint32_t* treeNodesOut ) {
	const uint32_t leaves = ( num_faces + 1 ) / 2;
	const uint32_t treeNodes = 2 * leaves - 1;
	DevBuf dLeft, dRight, dParent, dSize, dArrived, dBoxMin, dBoxMax;
	HIP_TRY( ctx, dLeft.alloc( sizeof( int ) * treeNodes ) );
	HIP_TRY( ctx, dRight.alloc( sizeof( int ) * treeNodes ) );
	HIP_TRY( ctx, dParent.alloc( sizeof( int ) * treeNodes ) );
	HIP_TRY( ctx, dSize.alloc( sizeof( unsigned ) * treeNodes ) );
	HIP_TRY( ctx, dArrived.alloc( sizeof( unsigned ) * treeNodes ) );
	HIP_TRY( ctx, dBoxMin.alloc( sizeof( float4 ) * treeNodes ) );
	HIP_TRY( ctx, dBoxMax.alloc( sizeof( float4 ) * treeNodes ) );
	HIP_TRY( ctx, hipMemsetAsync( dParent.get(), 0xFF, sizeof( int ) * treeNodes, ctx->stream ) );
	HIP_TRY( ctx, hipMemsetAsync( dArrived.get(), 0, sizeof( unsigned ) * treeNodes, ctx->stream ) );
	B.numLeaves = leaves;
	B.left = (int*) dLeft.get();
	B.right = (int*) dRight.get();
	B.parent = (int*) dParent.get();
	B.size = (unsigned*) dSize.get();
	B.arrived = (unsigned*) dArrived.get();
	B.boxMin = (float4*) dBoxMin.get();
	B.boxMax = (float4*) dBoxMax.get();
	const unsigned threads = 256;
	const unsigned leafBlocks = ( leaves + threads - 1 ) / threads;
	const unsigned nodeBlocks = ( treeNodes + threads - 1 ) / threads;

	if( leaves > 1 ) {
		hipLaunchKernelGGL( ptb::radixTree, dim3( leafBlocks ), dim3( threads ), 0, ctx->stream, B );
	}

	hipLaunchKernelGGL( ptb::boxesBottomUp, dim3( leafBlocks ), dim3( threads ), 0, ctx->stream, B );
	hipLaunchKernelGGL( ptb::flatten, dim3( nodeBlocks ), dim3( threads ), 0, ctx->stream, B );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );   // the buffers above are freed on return
	*treeNodesOut = treeNodes;
	return PBR_OK;
}

// locally-ordered clustering (csrc/bvh_build.hpp, PlocArrays): rounds of nearest-partner search, merge, compaction
int buildClustered( pbr_ctx* ctx, const ptb::BuildArrays& A, uint32_t num_faces, uint32_t* treeNodesOut ) {
	const uint32_t ids = 2 * num_faces - 1;
	DevBuf dLeft, dRight, dParent, dSize, dFaces, dBoxMin, dBoxMax, dClusters, dClustersNext, dNearest, dFlags, dScan, dTotals, dTemp;
	HIP_TRY( ctx, dLeft.alloc( sizeof( int ) * ids ) );
	HIP_TRY( ctx, dRight.alloc( sizeof( int ) * ids ) );
	HIP_TRY( ctx, dParent.alloc( sizeof( int ) * ids ) );
	HIP_TRY( ctx, dSize.alloc( sizeof( unsigned ) * ids ) );
	HIP_TRY( ctx, dFaces.alloc( sizeof( unsigned ) * ids ) );
	HIP_TRY( ctx, dBoxMin.alloc( sizeof( float4 ) * ids ) );
	HIP_TRY( ctx, dBoxMax.alloc( sizeof( float4 ) * ids ) );
	HIP_TRY( ctx, dClusters.alloc( sizeof( int ) * num_faces ) );
	HIP_TRY( ctx, dClustersNext.alloc( sizeof( int ) * num_faces ) );
	HIP_TRY( ctx, dNearest.alloc( sizeof( int ) * num_faces ) );
	HIP_TRY( ctx, dFlags.alloc( sizeof( unsigned long long ) * num_faces ) );
	HIP_TRY( ctx, dScan.alloc( sizeof( unsigned long long ) * num_faces ) );
	HIP_TRY( ctx, dTotals.alloc( sizeof( unsigned long long ) ) );

	ptb::PlocArrays B;
	B.vertices = A.vertices;
	B.facesV = A.facesV;
	B.facesN = A.facesN;
	B.numFaces = num_faces;
	B.keysSorted = A.keysSorted;
	B.left = (int*) dLeft.get();
	B.right = (int*) dRight.get();
	B.parent = (int*) dParent.get();
	B.size = (unsigned*) dSize.get();
	B.faces = (unsigned*) dFaces.get();
	B.boxMin = (float4*) dBoxMin.get();
	B.boxMax = (float4*) dBoxMax.get();
	B.clusters = (int*) dClusters.get();
	B.clustersNext = (int*) dClustersNext.get();
	B.nearest = (int*) dNearest.get();
	B.flags = (unsigned long long*) dFlags.get();
	B.scan = (unsigned long long*) dScan.get();
	B.totals = (unsigned long long*) dTotals.get();
	B.nodesOut = A.nodesOut;
	B.facesVOut = A.facesVOut;
	B.facesNOut = A.facesNOut;

	// The search radius.  For the reference's walk: 32 (round 2: 4 .. 64 within 3 % of each other on the Sponza- / Dragon-class
	// scenes, 32 the best on the hairball — where the numbers are noisy, because the stackless walk's fixed child order decides more
	// than the tree's area).  For a ray-ordered walk (round 5: the context is configured with pbr_config.traversal != 0) the child
	// order is out of the picture and the radius moves visits and speed monotonically — SMALLER is better: 3 gives 2183 / 2331 /
	// 1800 Msamples/s on the Sponza- / Dragon-class scenes and the hairball against 2112 / 2246 / 1414 at 32
	// (profiles/r05/experiments/ploc_radius_ordered_walk.txt).
	int radius = ( ctx->configured && ctx->cfg.traversal != 0 ) ? 3 : 32;

	if( ctx->knobs.plocRadius >= 1 ) {
		radius = ctx->knobs.plocRadius;
	}

	radius = std::min( std::max( radius, 1 ), PLOC_MAX_RADIUS );
	ctx->lastBvhRadius = radius;
	size_t tempBytes = 0;
	HIP_TRY( ctx, hipcub::DeviceScan::ExclusiveSum( nullptr, tempBytes, B.flags, B.scan, (int) num_faces, ctx->stream ) );
	HIP_TRY( ctx, dTemp.alloc( tempBytes ) );

	const unsigned threads = PLOC_THREADS;
	hipLaunchKernelGGL( ptb::plocInit, dim3( ( num_faces + threads - 1 ) / threads ), dim3( threads ), 0, ctx->stream, B );
	uint32_t count = num_faces, nextNode = num_faces;

	while( count > 1 ) {
		const dim3 grid( ( count + threads - 1 ) / threads );
		hipLaunchKernelGGL( ptb::plocNearest, grid, dim3( threads ), 0, ctx->stream, B, count, radius );
		hipLaunchKernelGGL( ptb::plocFlags, grid, dim3( threads ), 0, ctx->stream, B, count );
		HIP_TRY( ctx, hipcub::DeviceScan::ExclusiveSum( dTemp.get(), tempBytes, B.flags, B.scan, (int) count, ctx->stream ) );
		hipLaunchKernelGGL( ptb::plocMerge, grid, dim3( threads ), 0, ctx->stream, B, count, nextNode );
		HIP_TRY( ctx, hipGetLastError() );
		unsigned long long totals = 0;
		HIP_TRY( ctx, hipMemcpyAsync( &totals, B.totals, sizeof( totals ), hipMemcpyDeviceToHost, ctx->stream ) );
		HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
		const uint32_t merged = (uint32_t) ( totals >> 32 ), left = (uint32_t) ( totals & 0xFFFFFFFFull );

		if( merged == 0 || left + merged != count ) {
			// the smallest pair of a total order is always mutual — unless the boxes do not compare (NaN corners)
			return fail( ctx, PBR_EINVAL, "build_bvh: clustering made no progress with %u clusters left (non-finite vertices?)", count );
		}

		nextNode += merged;
		count = left;
		std::swap( B.clusters, B.clustersNext );
	}

	// one cluster is left: the root, the id created last (or face 0 of a single-face scene)
	uint32_t total = 0;
	HIP_TRY( ctx, hipMemcpyAsync( &total, B.size + ( nextNode - 1 ), sizeof( total ), hipMemcpyDeviceToHost, ctx->stream ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	hipLaunchKernelGGL( ptb::plocFlatten, dim3( ( nextNode + threads - 1 ) / threads ), dim3( threads ), 0, ctx->stream, B, nextNode, total );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	*treeNodesOut = total;
	return PBR_OK;
}

}  // namespace

// BVH on the device (csrc/bvh_build.hpp): Morton keys, radix sort, locally-ordered clustering by surface area,
// depth-first flattening into the reference's node format.
int pbr_build_bvh( pbr_ctx* ctx, const pbr_float4* vertices, uint32_t num_vertices, const pbr_uint4* facesV, const pbr_uint4* facesN,
                   uint32_t num_faces, pbr_bvh_node* nodes_out, uint32_t* num_nodes_out, pbr_uint4* facesV_out, pbr_uint4* facesN_out ) {
	if( ctx == nullptr || ctx->stream == nullptr ) {
		return PBR_EINVAL;
	}
	if( vertices == nullptr || facesV == nullptr || facesN == nullptr || nodes_out == nullptr || num_nodes_out == nullptr || facesV_out == nullptr || facesN_out == nullptr ) {
		return fail( ctx, PBR_EINVAL, "build_bvh: null argument" );
	}
	if( num_faces == 0 || num_vertices == 0 || num_faces > ( 1u << 24 ) ) {
		return fail( ctx, PBR_EINVAL, "build_bvh: needs 1 .. 2^24 faces and at least one vertex" );
	}

	for( uint32_t f = 0; f < num_faces; f++ ) {
		if( facesV[f].x >= num_vertices || facesV[f].y >= num_vertices || facesV[f].z >= num_vertices ) {
			return fail( ctx, PBR_EINVAL, "build_bvh: face %u: vertex index out of range", f );
		}
	}

	for( uint32_t v = 0; v < num_vertices; v++ ) {
		if( !std::isfinite( vertices[v].x ) || !std::isfinite( vertices[v].y ) || !std::isfinite( vertices[v].z ) ) {
			return fail( ctx, PBR_EINVAL, "build_bvh: vertex %u is not finite", v );
		}
	}

	const bool radix = ( ctx->knobs.bvhBuilder == 1 );   // round 1's radix tree; default: locally-ordered clustering

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	const uint32_t capacity = pbr_bvh_node_capacity( num_faces );
	DevBuf dVertices, dFacesV, dFacesN, dKeys, dKeysSorted, dBounds, dNodes, dFacesVOut, dFacesNOut, dTemp;
	HIP_TRY( ctx, dVertices.alloc( sizeof( pbr_float4 ) * num_vertices ) );
	HIP_TRY( ctx, dFacesV.alloc( sizeof( pbr_uint4 ) * num_faces ) );
	HIP_TRY( ctx, dFacesN.alloc( sizeof( pbr_uint4 ) * num_faces ) );
	HIP_TRY( ctx, dKeys.alloc( sizeof( unsigned long long ) * num_faces ) );
	HIP_TRY( ctx, dKeysSorted.alloc( sizeof( unsigned long long ) * num_faces ) );
	HIP_TRY( ctx, dBounds.alloc( sizeof( float ) * 8 ) );
	HIP_TRY( ctx, dNodes.alloc( sizeof( pbr_bvh_node ) * capacity ) );
	HIP_TRY( ctx, dFacesVOut.alloc( sizeof( pbr_uint4 ) * num_faces ) );
	HIP_TRY( ctx, dFacesNOut.alloc( sizeof( pbr_uint4 ) * num_faces ) );

	HIP_TRY( ctx, hipMemcpyAsync( dVertices.get(), vertices, sizeof( pbr_float4 ) * num_vertices, hipMemcpyHostToDevice, ctx->stream ) );
	HIP_TRY( ctx, hipMemcpyAsync( dFacesV.get(), facesV, sizeof( pbr_uint4 ) * num_faces, hipMemcpyHostToDevice, ctx->stream ) );
	HIP_TRY( ctx, hipMemcpyAsync( dFacesN.get(), facesN, sizeof( pbr_uint4 ) * num_faces, hipMemcpyHostToDevice, ctx->stream ) );
	// order-preserving unsigned images of +inf (minima) and -inf (maxima), see ptb::atomicMinFloat
	const unsigned bounds[8] = { 0xFF800000u, 0xFF800000u, 0xFF800000u, 0u, 0x007FFFFFu, 0x007FFFFFu, 0x007FFFFFu, 0u };
	HIP_TRY( ctx, hipMemcpyAsync( dBounds.get(), bounds, sizeof( bounds ), hipMemcpyHostToDevice, ctx->stream ) );

	ptb::BuildArrays B;
	std::memset( &B, 0, sizeof( B ) );
	B.vertices = (const pbr_float4*) dVertices.get();
	B.facesV = (const pbr_uint4*) dFacesV.get();
	B.facesN = (const pbr_uint4*) dFacesN.get();
	B.numFaces = num_faces;
	B.keys = (unsigned long long*) dKeys.get();
	B.keysSorted = (unsigned long long*) dKeysSorted.get();
	B.sceneMin = (float*) dBounds.get();
	B.sceneMax = (float*) dBounds.get() + 4;
	B.nodesOut = (pbr_bvh_node*) dNodes.get();
	B.facesVOut = (pbr_uint4*) dFacesVOut.get();
	B.facesNOut = (pbr_uint4*) dFacesNOut.get();

	const unsigned threads = 256;
	const unsigned faceBlocks = ( num_faces + threads - 1 ) / threads;

	HIP_TRY( ctx, hipEventRecord( ctx->evStart, ctx->stream ) );
	hipLaunchKernelGGL( ptb::centroidBounds, dim3( faceBlocks ), dim3( threads ), 0, ctx->stream, B );
	hipLaunchKernelGGL( ptb::mortonKeys, dim3( faceBlocks ), dim3( threads ), 0, ctx->stream, B );
	HIP_TRY( ctx, hipGetLastError() );

	size_t tempBytes = 0;
	HIP_TRY( ctx, hipcub::DeviceRadixSort::SortKeys( nullptr, tempBytes, B.keys, B.keysSorted, (int) num_faces, 0, 64, ctx->stream ) );
	HIP_TRY( ctx, dTemp.alloc( tempBytes ) );
	HIP_TRY( ctx, hipcub::DeviceRadixSort::SortKeys( dTemp.get(), tempBytes, B.keys, B.keysSorted, (int) num_faces, 0, 64, ctx->stream ) );

	uint32_t treeNodes = 0;
	PBR_TRY( radix ? buildRadixTree( ctx, B, num_faces, &treeNodes ) : buildClustered( ctx, B, num_faces, &treeNodes ) );

	HIP_TRY( ctx, hipEventRecord( ctx->evStop, ctx->stream ) );

	// a tree that is a single leaf has no container above it, but the walk starts at node 1 (pt_bvh.cl:84): give it a root
	pbr_bvh_node* firstTreeNode = ( treeNodes == 1 ) ? nodes_out + 1 : nodes_out;
	HIP_TRY( ctx, hipMemcpyAsync( firstTreeNode, dNodes.get(), sizeof( pbr_bvh_node ) * treeNodes, hipMemcpyDeviceToHost, ctx->stream ) );
	HIP_TRY( ctx, hipMemcpyAsync( facesV_out, dFacesVOut.get(), sizeof( pbr_uint4 ) * num_faces, hipMemcpyDeviceToHost, ctx->stream ) );
	HIP_TRY( ctx, hipMemcpyAsync( facesN_out, dFacesNOut.get(), sizeof( pbr_uint4 ) * num_faces, hipMemcpyDeviceToHost, ctx->stream ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );

	if( treeNodes == 1 ) {
		nodes_out[0] = nodes_out[1];
		nodes_out[0].bbMin.w = -1.0f;
		nodes_out[0].bbMax.w = -1.0f;
		*num_nodes_out = 2;
	}
	else {
		*num_nodes_out = treeNodes;
	}

	return timedTail( ctx );   // the stream is idle by now
}


// ---- diagnostic entry points (include/pbr_hip_diag.h) -----------------------------------

// The stage diagnostics in the native arithmetic (pt_diag_native.hip); null where that unit was not linked in (lab builds
// without flavour 2).
extern "C" const void* pt_diag_native_pick( int stage, uint32_t brdf ) __attribute__( ( weak ) );

namespace {

typedef void ( *DiagMathFn )( int, const float*, const float*, int, float* );
typedef void ( *DiagItemFn )( const ptk::DevParams, const float*, int, float* );
typedef void ( *DiagPlainFn )( const float*, int, float* );

// The kernel of a diagnostic stage (0 math, 1 BRDF, 2 new ray, 3 solveCubic, 4 Phong-tessellated face, 5 camera ray, 6 the
// intersection primitives, 7 the surface step) in the arithmetic of
// the configuration in force: the native flavour's after a successful pbr_configure with arith = PBR_ARITH_NATIVE, else (no configuration, or arith = exact) the
// exact one of this translation unit.  Null: the native unit is not linked in.
const void* diagKernel( const pbr_ctx* ctx, int stage, uint32_t brdf ) {
	if( ctx->configured && ctx->cfg.arith != 0 ) {
		return ( pt_diag_native_pick != nullptr ) ? pt_diag_native_pick( stage, brdf ) : nullptr;
	}
	switch( stage ) {
		case 0: return (const void*) ptk::diagMath;
		case 1: return ( brdf == 0 ) ? (const void*) ptk::diagBrdf<0> : (const void*) ptk::diagBrdf<1>;
		case 2: return ( brdf == 0 ) ? (const void*) ptk::diagNewRay<0> : (const void*) ptk::diagNewRay<1>;
		case 3: return (const void*) ptk::diagSolveCubic;
		case 5: return (const void*) ptk::diagCameraRay;
		case 6: return (const void*) ptk::diagIntersect;
		case 7: return ( brdf == 0 ) ? (const void*) ptk::diagSurfaceStep<0> : (const void*) ptk::diagSurfaceStep<1>;
		default: return (const void*) ptk::diagPhongFace;
	}
}

}  // namespace

int pbr_diag_math( pbr_ctx* ctx, int op, const float* x, const float* y, int n, float* out ) {
	if( ctx == nullptr || ctx->stream == nullptr || x == nullptr || out == nullptr || n <= 0 ) {
		return fail( ctx, PBR_EINVAL, "diag_math: bad argument" );
	}
	const DiagMathFn kernel = (DiagMathFn) diagKernel( ctx, 0, 0u );
	if( kernel == nullptr ) {
		return fail( ctx, PBR_ESTATE, "diag_math: this library was built without the native-arithmetic diagnostics" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	DevBuf dx, dy, dout;
	const size_t bytes = sizeof( float ) * (size_t) n;
	HIP_TRY( ctx, dx.alloc( bytes ) );
	HIP_TRY( ctx, dy.alloc( bytes ) );
	HIP_TRY( ctx, dout.alloc( bytes ) );
	HIP_TRY( ctx, hipMemcpy( dx.get(), x, bytes, hipMemcpyHostToDevice ) );
	HIP_TRY( ctx, hipMemcpy( dy.get(), ( y != nullptr ) ? y : x, bytes, hipMemcpyHostToDevice ) );
	hipLaunchKernelGGL( kernel, dim3( (unsigned) ( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, ctx->stream,
		op, (const float*) dx.get(), (const float*) dy.get(), n, (float*) dout.get() );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	HIP_TRY( ctx, hipMemcpy( out, dout.get(), bytes, hipMemcpyDeviceToHost ) );
	return PBR_OK;
}

int pbr_diag_trace( pbr_ctx* ctx, const float* rays, int n, float* out_t, int32_t* out_face, float* out_normal, uint32_t* out_counts ) {
	if( ctx == nullptr || !ctx->hasScene ) {
		return fail( ctx, PBR_ESTATE, "diag_trace before pbr_upload_scene" );
	}
	if( rays == nullptr || n <= 0 || out_t == nullptr || out_face == nullptr || out_normal == nullptr || out_counts == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_trace: bad argument" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	DevBuf dRays, dT, dFace, dNormal, dCounts;
	HIP_TRY( ctx, dRays.alloc( sizeof( float ) * 6 * (size_t) n ) );
	HIP_TRY( ctx, dT.alloc( sizeof( float ) * (size_t) n ) );
	HIP_TRY( ctx, dFace.alloc( sizeof( int ) * (size_t) n ) );
	HIP_TRY( ctx, dNormal.alloc( sizeof( float ) * 3 * (size_t) n ) );
	HIP_TRY( ctx, dCounts.alloc( sizeof( unsigned ) * 2 * (size_t) n ) );
	HIP_TRY( ctx, hipMemcpy( dRays.get(), rays, sizeof( float ) * 6 * (size_t) n, hipMemcpyHostToDevice ) );

	DevParams P;
	PBR_TRY( sceneParams( ctx, &P ) );
	const dim3 grid( (unsigned) ( ( n + 63 ) / 64 ) ), block( 64 );

	// Phong tessellation configured and the vertex-normal records uploaded: the PHONG build of the walk, as a render takes it
	const bool phong = ctx->configured && ctx->cfg.phong_tessellation > 0.0f && ctx->scene.dTriPN != nullptr;
	P.triPN = ctx->scene.dTriPN;
	P.phongAlpha = phong ? ctx->cfg.phong_tessellation : 0.0f;
	const void* kernel = ( ctx->scene.numLights > 0 )
		? ( phong ? (const void*) ptk::diagTrace<true, true> : (const void*) ptk::diagTrace<true, false> )
		: ( phong ? (const void*) ptk::diagTrace<false, true> : (const void*) ptk::diagTrace<false, false> );
	typedef void ( *DiagTraceFn )( const ptk::DevParams, const float*, int, float*, int*, float*, unsigned* );

	hipLaunchKernelGGL( (DiagTraceFn) kernel, grid, block, 0, ctx->stream, P, (const float*) dRays.get(), n,
		(float*) dT.get(), (int*) dFace.get(), (float*) dNormal.get(), (unsigned*) dCounts.get() );

	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	HIP_TRY( ctx, hipMemcpy( out_t, dT.get(), sizeof( float ) * (size_t) n, hipMemcpyDeviceToHost ) );
	HIP_TRY( ctx, hipMemcpy( out_face, dFace.get(), sizeof( int ) * (size_t) n, hipMemcpyDeviceToHost ) );
	HIP_TRY( ctx, hipMemcpy( out_normal, dNormal.get(), sizeof( float ) * 3 * (size_t) n, hipMemcpyDeviceToHost ) );
	HIP_TRY( ctx, hipMemcpy( out_counts, dCounts.get(), sizeof( unsigned ) * 2 * (size_t) n, hipMemcpyDeviceToHost ) );
	return PBR_OK;
}

namespace {

int diagPerItem( pbr_ctx* ctx, const float* in, int n, float* out, int inWidth, int outWidth, int stage ) {
	if( ctx == nullptr || !ctx->hasScene ) {
		return fail( ctx, PBR_ESTATE, "diag before pbr_upload_scene" );
	}
	if( in == nullptr || out == nullptr || n <= 0 ) {
		return fail( ctx, PBR_EINVAL, "diag: bad argument" );
	}
	const DiagItemFn kernel = (DiagItemFn) diagKernel( ctx, stage, ctx->scene.sceneBrdf );
	if( kernel == nullptr ) {
		return fail( ctx, PBR_ESTATE, "diag: this library was built without the native-arithmetic diagnostics" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	DevBuf dIn, dOut;
	HIP_TRY( ctx, dIn.alloc( sizeof( float ) * inWidth * (size_t) n ) );
	HIP_TRY( ctx, dOut.alloc( sizeof( float ) * outWidth * (size_t) n ) );
	HIP_TRY( ctx, hipMemcpy( dIn.get(), in, sizeof( float ) * inWidth * (size_t) n, hipMemcpyHostToDevice ) );

	DevParams P;
	PBR_TRY( sceneParams( ctx, &P ) );
	const dim3 grid( (unsigned) ( ( n + 63 ) / 64 ) ), block( 64 );

	hipLaunchKernelGGL( kernel, grid, block, 0, ctx->stream, P, (const float*) dIn.get(), n, (float*) dOut.get() );

	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	HIP_TRY( ctx, hipMemcpy( out, dOut.get(), sizeof( float ) * outWidth * (size_t) n, hipMemcpyDeviceToHost ) );
	return PBR_OK;
}

// pbr_diag_solve_cubic / pbr_diag_phong_face: items that need nothing of a scene
int diagPlain( pbr_ctx* ctx, const char* what, int stage, const float* in, int n, float* out, int inWidth, int outWidth ) {
	if( ctx == nullptr || ctx->stream == nullptr || in == nullptr || out == nullptr || n <= 0 ) {
		return fail( ctx, PBR_EINVAL, "%s: bad argument", what );
	}
	const DiagPlainFn kernel = (DiagPlainFn) diagKernel( ctx, stage, 0u );
	if( kernel == nullptr ) {
		return fail( ctx, PBR_ESTATE, "%s: this library was built without the native-arithmetic diagnostics", what );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	DevBuf dIn, dOut;
	HIP_TRY( ctx, dIn.alloc( sizeof( float ) * inWidth * (size_t) n ) );
	HIP_TRY( ctx, dOut.alloc( sizeof( float ) * outWidth * (size_t) n ) );
	HIP_TRY( ctx, hipMemcpy( dIn.get(), in, sizeof( float ) * inWidth * (size_t) n, hipMemcpyHostToDevice ) );
	hipLaunchKernelGGL( kernel, dim3( (unsigned) ( ( n + 63 ) / 64 ) ), dim3( 64 ), 0, ctx->stream, (const float*) dIn.get(), n, (float*) dOut.get() );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	HIP_TRY( ctx, hipMemcpy( out, dOut.get(), sizeof( float ) * outWidth * (size_t) n, hipMemcpyDeviceToHost ) );
	return PBR_OK;
}

}  // namespace

int pbr_diag_brdf( pbr_ctx* ctx, const float* in, int n, float* out ) {
	return diagPerItem( ctx, in, n, out, 16, 4, 1 );
}

int pbr_diag_solve_cubic( pbr_ctx* ctx, const float* in, int n, float* out ) {
	return diagPlain( ctx, "diag_solve_cubic", 3, in, n, out, 4, 4 );
}

int pbr_diag_phong_face( pbr_ctx* ctx, const float* in, int n, float* out ) {
	return diagPlain( ctx, "diag_phong_face", 4, in, n, out, 32, 4 );
}

int pbr_diag_new_ray( pbr_ctx* ctx, const float* in, int n, float* out ) {
	return diagPerItem( ctx, in, n, out, 12, 8, 2 );
}

int pbr_diag_surface_step( pbr_ctx* ctx, const float* in, int n, float* out ) {
	return diagPerItem( ctx, in, n, out, 24, 12, 7 );
}

int pbr_diag_camera_ray( pbr_ctx* ctx, float pxDim, const pbr_camera* cam, const float* in, int n, float* out ) {
	if( ctx == nullptr || ctx->stream == nullptr || cam == nullptr || in == nullptr || out == nullptr || n <= 0 ) {
		return fail( ctx, PBR_EINVAL, "diag_camera_ray: bad argument" );
	}
	if( !ctx->configured ) {
		return fail( ctx, PBR_ESTATE, "diag_camera_ray before pbr_configure" );
	}
	const DiagItemFn kernel = (DiagItemFn) diagKernel( ctx, 5, 0u );
	if( kernel == nullptr ) {
		return fail( ctx, PBR_ESTATE, "diag_camera_ray: this library was built without the native-arithmetic diagnostics" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	DevBuf dIn, dOut;
	HIP_TRY( ctx, dIn.alloc( sizeof( float ) * 8 * (size_t) n ) );
	HIP_TRY( ctx, dOut.alloc( sizeof( float ) * 8 * (size_t) n ) );
	HIP_TRY( ctx, hipMemcpy( dIn.get(), in, sizeof( float ) * 8 * (size_t) n, hipMemcpyHostToDevice ) );

	// the camera as beginRender hands it to a render's kernels; initRay reads nothing else of P
	DevParams P;
	std::memset( &P, 0, sizeof( P ) );
	setCamera( &P, cam, (int) ctx->cfg.width, (int) ctx->cfg.height, pxDim );
	P.aperture = cam->lense[0] / cam->lense[1];
	P.antiAliasing = ctx->cfg.anti_aliasing;

	hipLaunchKernelGGL( kernel, dim3( (unsigned) ( ( n + 63 ) / 64 ) ), dim3( 64 ), 0, ctx->stream, P, (const float*) dIn.get(), n, (float*) dOut.get() );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	HIP_TRY( ctx, hipMemcpy( out, dOut.get(), sizeof( float ) * 8 * (size_t) n, hipMemcpyDeviceToHost ) );
	return PBR_OK;
}

int pbr_diag_intersect( pbr_ctx* ctx, int op, const float* in, int n, float* out ) {
	if( ctx == nullptr || ctx->stream == nullptr || in == nullptr || out == nullptr || n <= 0 || op < 0 || op > 2 ) {
		return fail( ctx, PBR_EINVAL, "diag_intersect: bad argument" );
	}
	typedef void ( *DiagOpFn )( int, const float*, int, float* );
	const DiagOpFn kernel = (DiagOpFn) diagKernel( ctx, 6, 0u );
	if( kernel == nullptr ) {
		return fail( ctx, PBR_ESTATE, "diag_intersect: this library was built without the native-arithmetic diagnostics" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	DevBuf dIn, dOut;
	HIP_TRY( ctx, dIn.alloc( sizeof( float ) * 24 * (size_t) n ) );
	HIP_TRY( ctx, dOut.alloc( sizeof( float ) * 4 * (size_t) n ) );
	HIP_TRY( ctx, hipMemcpy( dIn.get(), in, sizeof( float ) * 24 * (size_t) n, hipMemcpyHostToDevice ) );
	hipLaunchKernelGGL( kernel, dim3( (unsigned) ( ( n + 63 ) / 64 ) ), dim3( 64 ), 0, ctx->stream, op, (const float*) dIn.get(), n, (float*) dOut.get() );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	HIP_TRY( ctx, hipMemcpy( out, dOut.get(), sizeof( float ) * 4 * (size_t) n, hipMemcpyDeviceToHost ) );
	return PBR_OK;
}

// Experimental: stream n rays {ox,oy,oz,_, dx,dy,dz,_} through the traversal-only probe `repeats`
// times; returns the best kernel time in *ms_out and the last hits in out (n x {t, face-bits}).
int pbr_diag_trace_stream( pbr_ctx* ctx, int mode, const float* rays8, uint32_t n, int repeats, float* out2, double* ms_out ) {
	if( ctx == nullptr || !ctx->hasScene || rays8 == nullptr || n == 0 || out2 == nullptr || ms_out == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_trace_stream: bad argument / no scene" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	DevBuf dRays, dOut;
	HIP_TRY( ctx, dRays.alloc( sizeof( float ) * 8 * (size_t) n ) );
	HIP_TRY( ctx, dOut.alloc( sizeof( float ) * 2 * (size_t) n ) );
	HIP_TRY( ctx, hipMemcpy( dRays.get(), rays8, sizeof( float ) * 8 * (size_t) n, hipMemcpyHostToDevice ) );

	uint32_t hotAvail = 0;
	DevParams P;
	PBR_TRY( sceneParams( ctx, &P, &hotAvail ) );
	P.workCounter = ctx->dWork;
	P.counters = ctx->dCounters;
	ctx->workClean = false;   // this probe uses the queue heads its own way
	double best = 1e30;

	for( int r = 0; r < repeats; r++ ) {
		HIP_TRY( ctx, hipMemsetAsync( ctx->dWork, 0, kWorkBytes, ctx->stream ) );
		HIP_TRY( ctx, hipEventRecord( ctx->evStart, ctx->stream ) );

		// mode = number of hot nodes to stage in LDS (0 = none); 8 waves / SIMD => 2048 threads per CU
		const int blocksPerCU = 2048 / PBR_BLOCK;
		size_t slots = std::min<size_t>( (size_t) mode, hotAvail );
		slots = std::min<size_t>( slots, ( 160 * 1024 / (size_t) blocksPerCU - 256 ) / 32 );
		slots &= ( P.walkScheme == 3 ) ? ~(size_t) 1 : ~(size_t) 0;      // compact records are two slots each
		P.numHot = (int) slots;
		P.numHotBytes = (int) slots * 32;
		const dim3 grid( (unsigned) ( ctx->numCUs * blocksPerCU ) ), block( PBR_BLOCK );

		if( slots == 0 ) {
			hipLaunchKernelGGL( ptk::diagTraceStream<false>, grid, block, 0, ctx->stream, P, (const float4*) dRays.get(), n, (float2*) dOut.get() );
		}
		else {
			HIP_TRY( ctx, hipFuncSetAttribute( (const void*) ptk::diagTraceStream<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) ( slots * 32 ) ) );
			hipLaunchKernelGGL( ptk::diagTraceStream<true>, grid, block, slots * 32, ctx->stream, P, (const float4*) dRays.get(), n, (float2*) dOut.get() );
		}

		HIP_TRY( ctx, hipGetLastError() );
		HIP_TRY( ctx, hipEventRecord( ctx->evStop, ctx->stream ) );
		HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
		float ms = 0.0f;
		HIP_TRY( ctx, hipEventElapsedTime( &ms, ctx->evStart, ctx->evStop ) );
		best = ( ms < best ) ? ms : best;
	}

	HIP_TRY( ctx, hipMemcpy( out2, dOut.get(), sizeof( float ) * 2 * (size_t) n, hipMemcpyDeviceToHost ) );
	*ms_out = best;
	return PBR_OK;
}

namespace {

// pbr_diag_trace_walk's staged prefix, clamped as pbr_diag_trace_stream clamps its own: the ranked prefix, a block's share of LDS
// at two blocks per CU, whole compact records
size_t walkSlots( int lds_slots, uint32_t hotAvail, int walkScheme ) {
	const int blocksPerCU = 2048 / PBR_BLOCK;
	size_t slots = std::min<size_t>( (size_t) lds_slots, hotAvail );
	slots = std::min<size_t>( slots, ( 160 * 1024 / (size_t) blocksPerCU - 256 ) / 32 );
	slots &= ( walkScheme == 3 ) ? ~(size_t) 1 : ~(size_t) 0;
	return slots;
}

}  // namespace

int pbr_diag_trace_walk_slots( pbr_ctx* ctx, int lds_slots, uint32_t* slots, uint32_t* hot_slots ) {
	if( ctx == nullptr || !ctx->hasScene ) {
		return fail( ctx, PBR_ESTATE, "diag_trace_walk_slots before pbr_upload_scene" );
	}
	if( lds_slots < 0 || slots == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_trace_walk_slots: bad argument" );
	}

	uint32_t hotAvail = 0;
	DevParams P;
	PBR_TRY( sceneParams( ctx, &P, &hotAvail ) );
	*slots = (uint32_t) walkSlots( lds_slots, hotAvail, P.walkScheme );

	if( hot_slots != nullptr ) {
		*hot_slots = hotAvail;
	}

	return PBR_OK;
}

// One chosen ray per thread through the walk a lock-step render runs (pt_walk_diag.hpp): the kernel of the context's build
// flavour, the staged prefix clamped as above, the park share of a render's plan.
int pbr_diag_trace_walk( pbr_ctx* ctx, int anyhit, int lds_slots, const float* rays8, uint32_t n,
                         float* out_t, int32_t* out_face, float* out_normal, uint32_t* out_counts ) {
	if( ctx == nullptr || !ctx->hasScene ) {
		return fail( ctx, PBR_ESTATE, "diag_trace_walk before pbr_upload_scene" );
	}
	if( rays8 == nullptr || n == 0 || n > ( 1u << 24 ) || lds_slots < 0 || out_t == nullptr || out_face == nullptr || out_normal == nullptr || out_counts == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_trace_walk: bad argument" );
	}

	const int flavour = ctx->configured ? flavourOf( ctx->cfg ) : 0;
	const pti_picker pick = kPickers[flavour][PTI_WALK];

	if( pick == nullptr ) {
		return fail( ctx, PBR_ESTATE, "diag_trace_walk: this library was built without the per-ray walk of flavour %d", flavour );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	DevBuf dRays, dT, dFace, dNormal, dCounts;
	HIP_TRY( ctx, dRays.alloc( sizeof( float ) * 8 * (size_t) n ) );
	HIP_TRY( ctx, dT.alloc( sizeof( float ) * (size_t) n ) );
	HIP_TRY( ctx, dFace.alloc( sizeof( int ) * (size_t) n ) );
	HIP_TRY( ctx, dNormal.alloc( sizeof( float ) * 3 * (size_t) n ) );
	HIP_TRY( ctx, dCounts.alloc( sizeof( unsigned ) * 2 * (size_t) n ) );
	HIP_TRY( ctx, hipMemcpy( dRays.get(), rays8, sizeof( float ) * 8 * (size_t) n, hipMemcpyHostToDevice ) );

	uint32_t hotAvail = 0;
	DevParams P;
	PBR_TRY( sceneParams( ctx, &P, &hotAvail ) );

	// Phong tessellation and lights as pbr_diag_trace takes them
	const bool phong = ctx->configured && ctx->cfg.phong_tessellation > 0.0f && ctx->scene.dTriPN != nullptr;
	P.triPN = ctx->scene.dTriPN;
	P.phongAlpha = phong ? ctx->cfg.phong_tessellation : 0.0f;
	// the park share of a render's plan (makePlan)
	P.parkEighths = ( ctx->scene.numNodes >= kWideMinNodes ) ? 4 : 6;

	if( ctx->knobs.parkEighths >= 0 ) {
		P.parkEighths = std::min( 8, ctx->knobs.parkEighths );
	}

	// the staged prefix as pbr_diag_trace_stream clamps it: the ranked prefix, a block's share of LDS, whole compact records
	const size_t slots = walkSlots( lds_slots, hotAvail, P.walkScheme );
	P.numHot = (int) slots;
	P.numHotBytes = (int) slots * 32;

	typedef void ( *WalkFn )( const ptk::DevParams, const float4*, unsigned, float*, int*, float*, unsigned* );
	const WalkFn kernel = (WalkFn) pick( ( anyhit ? 1u : 0u ) | ( slots > 0 ? 2u : 0u ), phong ? 1 : 0, ( ctx->scene.numLights > 0 ) ? 1 : 0 );

	if( slots > 0 ) {
		HIP_TRY( ctx, hipFuncSetAttribute( (const void*) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) ( slots * 32 ) ) );
	}

	// the kernels' error flags are of this launch (host-mapped memory; no launch of this context is in flight here)
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );

	for( int k = 0; k < 4; k++ ) {
		( (volatile unsigned*) ctx->dGuard )[k] = 0u;
	}

	const dim3 grid( ( n + PBR_BLOCK - 1 ) / PBR_BLOCK ), block( PBR_BLOCK );
	hipLaunchKernelGGL( kernel, grid, block, slots * 32, ctx->stream, P, (const float4*) dRays.get(), n,
		(float*) dT.get(), (int*) dFace.get(), (float*) dNormal.get(), (unsigned*) dCounts.get() );
	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	PBR_TRY( checkGuard( ctx ) );
	HIP_TRY( ctx, hipMemcpy( out_t, dT.get(), sizeof( float ) * (size_t) n, hipMemcpyDeviceToHost ) );
	HIP_TRY( ctx, hipMemcpy( out_face, dFace.get(), sizeof( int ) * (size_t) n, hipMemcpyDeviceToHost ) );
	HIP_TRY( ctx, hipMemcpy( out_normal, dNormal.get(), sizeof( float ) * 3 * (size_t) n, hipMemcpyDeviceToHost ) );
	HIP_TRY( ctx, hipMemcpy( out_counts, dCounts.get(), sizeof( unsigned ) * 2 * (size_t) n, hipMemcpyDeviceToHost ) );
	return PBR_OK;
}


// Counter calibration: allocate a zero-filled table of table_bytes, read `reads` elements / records
// in the given pattern (0 stream, 1 random 16 B, 2 random 32 B); reports the kernel time.  Run it
// under rocprofv3 --pmc to see what the memory counters say about a KNOWN amount of traffic.
int pbr_diag_calibrate( pbr_ctx* ctx, int mode, uint64_t table_bytes, uint64_t reads, double* ms_out ) {
	if( ctx == nullptr || ctx->stream == nullptr || mode < 0 || mode > 2 || table_bytes < 4096 || reads == 0 || ms_out == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_calibrate: bad argument" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	DevBuf table, sink;
	HIP_TRY( ctx, table.alloc( (size_t) table_bytes ) );
	HIP_TRY( ctx, sink.alloc( 64 ) );
	HIP_TRY( ctx, hipMemset( table.get(), 0, (size_t) table_bytes ) );
	HIP_TRY( ctx, hipDeviceSynchronize() );

	const unsigned long long count = table_bytes / 16;
	const unsigned blocks = (unsigned) ctx->numCUs * 8;
	const unsigned long long threads = (unsigned long long) blocks * 256;
	const unsigned steps = (unsigned) ( ( reads + threads - 1 ) / threads );

	HIP_TRY( ctx, hipEventRecord( ctx->evStart, ctx->stream ) );

	if( mode == 0 ) {
		hipLaunchKernelGGL( ptk::diagCalibrate<0>, dim3( blocks ), dim3( 256 ), 0, ctx->stream, (const float4*) table.get(), count, steps, (float*) sink.get() );
	}
	else if( mode == 1 ) {
		hipLaunchKernelGGL( ptk::diagCalibrate<1>, dim3( blocks ), dim3( 256 ), 0, ctx->stream, (const float4*) table.get(), count, steps, (float*) sink.get() );
	}
	else {
		hipLaunchKernelGGL( ptk::diagCalibrate<2>, dim3( blocks ), dim3( 256 ), 0, ctx->stream, (const float4*) table.get(), count, steps, (float*) sink.get() );
	}

	HIP_TRY( ctx, hipGetLastError() );
	HIP_TRY( ctx, hipEventRecord( ctx->evStop, ctx->stream ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	float ms = 0.0f;
	HIP_TRY( ctx, hipEventElapsedTime( &ms, ctx->evStart, ctx->evStop ) );
	*ms_out = (double) ms * 1.0;
	return PBR_OK;
}

int pbr_diag_tune_budget( pbr_ctx* ctx, uint32_t* frames ) {
	if( ctx == nullptr || frames == nullptr ) {
		return PBR_EINVAL;
	}
	if( !ctx->configured ) {
		return fail( ctx, PBR_ESTATE, "tune budget before pbr_configure" );
	}

	*frames = ctx->tuner.budgetFrames();
	return PBR_OK;
}

int pbr_diag_last_plan( pbr_ctx* ctx, char* name, size_t capacity, int* tuned ) {
	if( ctx == nullptr || name == nullptr || capacity == 0 ) {
		return fail( ctx, PBR_EINVAL, "diag_last_plan: null argument" );
	}

	std::snprintf( name, capacity, "%s", ctx->lastPlan );

	if( tuned != nullptr ) {
		*tuned = ctx->tuner.tunedPlan();
	}

	return PBR_OK;
}

int pbr_diag_last_deal( pbr_ctx* ctx, char* name, size_t capacity, int* learnt ) {
	if( ctx == nullptr || name == nullptr || capacity == 0 ) {
		return fail( ctx, PBR_EINVAL, "diag_last_deal: null argument" );
	}

	std::snprintf( name, capacity, "%s", ctx->lastDeal );

	if( learnt != nullptr ) {
		*learnt = ctx->costLearnt ? 1 : 0;
	}

	return PBR_OK;
}

int pbr_diag_bvh_build_info( pbr_ctx* ctx, int* radius ) {
	if( ctx == nullptr || radius == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_bvh_build_info: null argument" );
	}

	*radius = ctx->lastBvhRadius;
	return PBR_OK;
}

int pbr_diag_scene_bytes( pbr_ctx* ctx, uint64_t out[3] ) {
	if( ctx == nullptr || out == nullptr || !ctx->hasScene ) {
		return fail( ctx, PBR_ESTATE, "diag_scene_bytes: no scene" );
	}

	out[0] = ctx->scene.dNodes.bytes();
	out[1] = ctx->scene.walk.dNodesWalk.bytes();
	out[2] = ctx->scene.dTris.bytes();
	return PBR_OK;
}

int pbr_diag_refit_info( pbr_ctx* ctx, uint64_t out[8], double* upload_ms, char* why, size_t capacity ) {
	if( ctx == nullptr || out == nullptr || !ctx->hasScene ) {
		return fail( ctx, PBR_ESTATE, "diag_refit_info: no scene" );
	}

	out[0] = ctx->scene.refit.nested ? 1 : 0;
	out[1] = ctx->scene.refit.subtreeCap;
	out[2] = ctx->scene.refitGroups;
	out[3] = ctx->scene.refitSubtrees;
	out[4] = ctx->scene.refitTopNodes;
	out[5] = ctx->scene.refitLevels;
	out[6] = ctx->scene.refitBytes();
	out[7] = ctx->scene.refitUpdates;

	if( upload_ms != nullptr ) {
		*upload_ms = ctx->lastRefitUploadMs;
	}
	if( why != nullptr && capacity > 0 ) {
		std::snprintf( why, capacity, "%s", ctx->scene.refit.why.c_str() );
	}

	return PBR_OK;
}

int pbr_diag_patch_refit_info( pbr_ctx* ctx, uint64_t out[4], float* alpha ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}
	if( out == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_patch_refit_info: null out" );
	}
	if( !ctx->hasScene ) {
		return fail( ctx, PBR_ESTATE, "diag_patch_refit_info: no scene" );
	}

	out[0] = ( ctx->scene.dTriPN != nullptr ) ? 1 : 0;
	out[1] = ctx->scene.dPatchFacesN.bytes() + ctx->scene.dPatchNormals.bytes() + ctx->scene.dFaceBoxes.bytes();
	out[2] = ctx->scene.geometryUpdates;
	out[3] = updateWasGeometry( ctx->lastUpdate ) ? 1 : 0;

	if( alpha != nullptr ) {
		*alpha = ctx->scene.patchAlpha;
	}

	return PBR_OK;
}

int pbr_diag_read_patches( pbr_ctx* ctx, pbr_float4* out, uint32_t capacity, uint32_t* count ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}
	if( !ctx->hasScene || ctx->scene.dTriPN == nullptr ) {
		return fail( ctx, PBR_ESTATE, "diag_read_patches: no scene, or one without usable vertex normals (no Phong patches)" );
	}
	if( count == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_read_patches: null count" );
	}

	*count = ctx->scene.numFaces * 6u;

	if( out == nullptr ) {
		return PBR_OK;
	}
	if( capacity < *count ) {
		return fail( ctx, PBR_EINVAL, "diag_read_patches: room for %u quads, the patches hold %u", capacity, *count );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	HIP_TRY( ctx, hipMemcpy( out, ctx->scene.dTriPN, sizeof( pbr_float4 ) * (size_t) *count, hipMemcpyDeviceToHost ) );
	return PBR_OK;
}

int pbr_diag_read_walk( pbr_ctx* ctx, void* out, uint64_t capacity, uint64_t* bytes, int first[8], uint32_t* hot_slots ) {
	if( ctx == nullptr ) {
		return PBR_EINVAL;
	}
	if( !ctx->hasScene || ctx->scene.walk.dNodesWalk == nullptr || ctx->scene.walk.walkBuilt == 0 ) {
		return fail( ctx, PBR_ESTATE, "diag_read_walk: no ray-ordered stream is built" );
	}
	if( bytes == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_read_walk: null bytes" );
	}

	*bytes = ctx->scene.walk.dNodesWalk.bytes();

	if( first != nullptr ) {
		std::memcpy( first, ctx->scene.walk.walkFirst, sizeof( ctx->scene.walk.walkFirst ) );
	}
	if( hot_slots != nullptr ) {
		*hot_slots = ctx->scene.walk.walkHotAvail;
	}
	if( out == nullptr ) {
		return PBR_OK;
	}
	if( capacity < ctx->scene.walk.dNodesWalk.bytes() ) {
		return fail( ctx, PBR_EINVAL, "diag_read_walk: room for %llu bytes, the streams hold %llu", (unsigned long long) capacity, (unsigned long long) ctx->scene.walk.dNodesWalk.bytes() );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	HIP_TRY( ctx, hipStreamSynchronize( ctx->stream ) );
	HIP_TRY( ctx, hipMemcpy( out, ctx->scene.walk.dNodesWalk, ctx->scene.walk.dNodesWalk.bytes(), hipMemcpyDeviceToHost ) );
	return PBR_OK;
}

int pbr_diag_relink_info( pbr_ctx* ctx, uint64_t out[4], double* ms ) {
	if( ctx == nullptr || out == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_relink_info: null argument" );
	}

	out[0] = ctx->scene.walk.dRelink.bytes();
	out[1] = ( ctx->scene.walk.dRelink != nullptr ) ? ctx->scene.walk.relinkLevels : 0;
	out[2] = ctx->lastRelinkLaunches;
	out[3] = ctx->lastRelinked ? 1 : 0;

	if( ms != nullptr ) {
		*ms = ctx->lastRelinkMs;
	}

	return PBR_OK;
}

int pbr_diag_last_kernel( pbr_ctx* ctx, char* name, size_t capacity ) {
	if( ctx == nullptr || name == nullptr || capacity == 0 ) {
		return fail( ctx, PBR_EINVAL, "diag_last_kernel: null argument" );
	}

	std::snprintf( name, capacity, "%s", ctx->lastKernel );
	return PBR_OK;
}

int pbr_diag_launch_fit( pbr_ctx* ctx, double* fixed_ms, double* per_frame_ms ) {
	if( ctx == nullptr || fixed_ms == nullptr || per_frame_ms == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_launch_fit: null argument" );
	}

	const int plan = ( ctx->pinnedPlan >= 0 ) ? ctx->pinnedPlan : ctx->tuner.tunedPlan();
	return ctx->tuner.fit( plan, fixed_ms, per_frame_ms ) ? PBR_OK : fail( ctx, PBR_ESTATE, "diag_launch_fit: the tuner holds no two-length fit for the plan in use (pinned before it tuned, or launches of one length only)" );
}

int pbr_diag_set_knob( pbr_ctx* ctx, const char* name, int value ) {
	if( ctx == nullptr || name == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_set_knob: null argument" );
	}

	Knobs& k = ctx->knobs;
	const struct { const char* name; int* slot; } table[] = {
		{ "lds_slots", &k.ldsSlots }, { "blocks_per_cu", &k.blocksPerCU }, { "ph_park", &k.phPark }, { "ph_shade", &k.phShade },
		{ "park_eighths", &k.parkEighths }, { "drain_mode", &k.drainMode }, { "refill_batch", &k.refillBatch },
		{ "chunk_frames", &k.chunkFrames }, { "face_normals", &k.faceNormals }, { "bvh_builder", &k.bvhBuilder },
		{ "ploc_radius", &k.plocRadius }, { "tune_log", &k.tuneLog }, { "deal_order", &k.dealOrder }, { "chain_layout", &k.chainLayout },
		{ "display_merge", &k.displayMerge },
	};

	for( const auto& entry : table ) {
		if( std::strcmp( entry.name, name ) == 0 ) {
			*entry.slot = value;
			replan( ctx );
			return PBR_OK;
		}
	}

	return fail( ctx, PBR_EINVAL, "diag_set_knob: unknown knob '%s'", name );
}

int pbr_diag_get_tile_order( pbr_ctx* ctx, int which, uint32_t* order, uint32_t capacity, uint32_t* count, uint32_t band_first[PT_BANDS + 1] ) {
	if( ctx == nullptr || !ctx->configured ) {
		return fail( ctx, PBR_ESTATE, "diag_get_tile_order before pbr_configure" );
	}
	if( which != 0 && !ctx->costLearnt ) {
		return fail( ctx, PBR_ESTATE, "diag_get_tile_order: no cost order has been learnt yet (it is built after the first render)" );
	}

	const DealTable& table = ctx->images.deal[( which == kDealCostClasses || which == kDealExpensiveLast ) ? which : kDealSpatial];
	const uint32_t n = (uint32_t) table.host.size();

	if( count != nullptr ) {
		*count = n;
	}

	if( band_first != nullptr ) {
		for( int band = 0; band <= PT_BANDS; band++ ) {
			band_first[band] = table.first[band];
		}
	}

	if( order != nullptr ) {
		if( capacity < n ) {
			return fail( ctx, PBR_EINVAL, "diag_get_tile_order: %u entries do not fit a buffer of %u", n, capacity );
		}

		std::memcpy( order, table.host.data(), sizeof( uint32_t ) * n );
	}

	return PBR_OK;
}

int pbr_diag_set_tile_order( pbr_ctx* ctx, const uint32_t* order, uint32_t count, const uint32_t* band_first ) {
	if( ctx == nullptr || !ctx->configured ) {
		return fail( ctx, PBR_ESTATE, "diag_set_tile_order before pbr_configure" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	std::vector<unsigned> spatial;
	unsigned spatialFirst[PT_BANDS + 1];
	spatialTileOrder( ctx->queueGrid, ctx->numLocalTiles, PT_BANDS, &spatial, spatialFirst );
	DealTable& table = ctx->images.deal[kDealSpatial];

	if( order == nullptr ) {
		table.host = spatial;
		std::memcpy( table.first, spatialFirst, sizeof( spatialFirst ) );
		ctx->orderPinned = false;
		return uploadTileOrder( ctx );
	}

	std::string why;

	if( tileOrderCheck( order, count, band_first, spatial, spatialFirst, PT_BANDS, &why ) != PBR_OK ) {
		return fail( ctx, PBR_EINVAL, "%s", why.c_str() );
	}

	table.host.assign( order, order + count );
	std::memcpy( table.first, ( band_first != nullptr ) ? band_first : spatialFirst, sizeof( spatialFirst ) );
	ctx->orderPinned = true;
	return uploadTileOrder( ctx );
}

int pbr_diag_pin_plan( pbr_ctx* ctx, int plan ) {
	if( ctx == nullptr || plan < -1 || plan > 6 ) {
		return fail( ctx, PBR_EINVAL, "diag_pin_plan: plan must be -1 (auto-tune) or 0..6" );
	}

	ctx->pinnedPlan = plan;
	return PBR_OK;
}

int pbr_diag_last_trace( pbr_ctx* ctx, double* trace_ms, uint32_t* launches ) {
	if( ctx == nullptr || trace_ms == nullptr || launches == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_last_trace: null argument" );
	}

	*trace_ms = ctx->lastTraceMs;
	*launches = ctx->lastTraceLaunches;
	return PBR_OK;
}

int pbr_diag_last_focus_chain( pbr_ctx* ctx, double* ms ) {
	if( ctx == nullptr || ms == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_last_focus_chain: null argument" );
	}

	*ms = ctx->lastChainMs;
	return PBR_OK;
}

int pbr_diag_last_adaptive( pbr_ctx* ctx, uint32_t* rounds, uint64_t* units_traced, double* fold_ms ) {
	if( ctx == nullptr || rounds == nullptr || units_traced == nullptr || fold_ms == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_last_adaptive: null argument" );
	}
	if( !ctx->adaptiveStats ) {
		return fail( ctx, PBR_ESTATE, "diag_last_adaptive before pbr_render_adaptive" );
	}

	*rounds = ctx->lastAdaptiveRounds;
	*units_traced = ctx->lastAdaptiveUnits;
	*fold_ms = ctx->lastAdaptiveFoldMs;
	return PBR_OK;
}

int pbr_diag_raw_counters( pbr_ctx* ctx, uint64_t out[16] ) {
	if( ctx == nullptr || out == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_raw_counters: null argument" );
	}

	HIP_TRY( ctx, hipSetDevice( ctx->device ) );
	HIP_TRY( ctx, hipMemcpy( out, ctx->dCounters, sizeof( uint64_t ) * kCounterSlots, hipMemcpyDeviceToHost ) );
	return PBR_OK;
}

int pbr_diag_guard_trips( pbr_ctx* ctx, uint32_t out[3] ) {
	if( ctx == nullptr || ctx->stream == nullptr || out == nullptr ) {
		return fail( ctx, PBR_EINVAL, "diag_guard_trips: bad argument" );
	}

	const volatile unsigned* host = ctx->dGuard;
	out[0] = host[0];
	out[1] = host[1];
	out[2] = host[2];
	return PBR_OK;
}

}  // extern "C"
