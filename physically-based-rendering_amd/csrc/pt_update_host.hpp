// pt_update_host.hpp — what the eight update calls (pbr_update_vertices, pbr_update_geometry, pbr_update_transforms,
// pbr_update_skin, pbr_update_morph, pbr_update_pose, pbr_update_skin_dq, pbr_update_pose_dq; include/pbr_hip.h) decide before and
// around their launches, and what the context remembers of the last one.  Host code only, no HIP: pbr_hip.hip gathers the facts from the context and calls this
// unit, tests/update_plan_driver.cpp builds it with a plain C++17 compiler.
//
// A call is refused in three stages, and the first refusal wins:
//   1  admitKind     the kind's own state: no morph / no skin / two generations / no parts / no scene
//   2                the kind's argument check (checkMorphWeights, checkSkinMatrices, checkSkinDualQuats, checkTransforms,
//                    checkRefitVertices, checkRefitNormals — each in its own host unit; they also fill the pinned tables), run
//                    by the caller
//   3  admitShared   what every update shares: a tree that is not nested, an ordered walk without pbr_refit_ordered_walk,
//                    pbr_update_vertices under Phong tessellation, new normals for a scene without patches
// planUpdate then says what the accepted call launches.
#pragma once

#include <cstdint>
#include <string>

#include "pt_scene_pack.hpp"

// The kinds of update, and `None`: no update since the upload.  The context keeps the kind of the most recent successful one.
// SkinDQ and PoseDQ are Skin and Pose with dual quaternions for the bones (pt_skin_dq_host.hpp); new kinds are appended.
enum class UpdateKind : uint32_t { None = 0, Vertices, Geometry, Transforms, Skin, Morph, Pose, SkinDQ, PoseDQ };

// pbr_configure's state rule and pbr_diag_patch_refit_info: the last update was "a pbr_update_geometry" — every kind but
// pbr_update_vertices is one, it brings or computes the normals' side too
inline bool updateWasGeometry( UpdateKind last ) {
	return last != UpdateKind::None && last != UpdateKind::Vertices;
}

// pbr_diag_morph_info: 0 none of the two, 1 a pbr_update_morph, 2 a pbr_update_pose
inline uint32_t updateMorphCode( UpdateKind last ) {
	return ( last == UpdateKind::Morph ) ? 1u : ( last == UpdateKind::Pose ) ? 2u : 0u;
}

// pbr_diag_skin_dq_info: 0 none of the two, 1 a pbr_update_skin_dq, 2 a pbr_update_pose_dq
inline uint32_t updateDualQuatCode( UpdateKind last ) {
	return ( last == UpdateKind::SkinDQ ) ? 1u : ( last == UpdateKind::PoseDQ ) ? 2u : 0u;
}

inline const char* updateCall( UpdateKind kind ) {
	static const char* const names[] = { "", "pbr_update_vertices", "pbr_update_geometry", "pbr_update_transforms", "pbr_update_skin", "pbr_update_morph", "pbr_update_pose",
	                                     "pbr_update_skin_dq", "pbr_update_pose_dq" };
	return names[(uint32_t) kind];
}

// What the decisions read of the context.
struct UpdateFacts {
	bool hasScene = false;
	bool nested = false;               // RefitPlan's verdict ...
	const char* why = "";              // ... and its reason
	bool configured = false;
	uint32_t traversal = 0;            // pbr_config's, meaningful while configured
	float phongTessellation = 0.0f;    // likewise
	bool refitOrdered = false;         // pbr_refit_ordered_walk
	bool hasPatches = false;           // the upload kept exact vertices + vertex normals per face (dTriPN)
	bool walkBuilt = false;            // the ordered records are there and hold the configured traversal's layout
	uint32_t numParts = 0, numBones = 0, numMorphTargets = 0;
	uint64_t skinGeneration = 0, morphGeneration = 0;   // the geometry pbr_set_skin / pbr_set_morph captured
	bool partNormals = false, skinNormals = false, morphNormals = false;   // the set call was given the normals' side too
	bool tracking = false, history = false, moved = false;                 // TemporalPolicy's
};

// Stage 1.  PBR_OK, or the status with the message in *why.
inline int admitKind( UpdateKind kind, const UpdateFacts& f, std::string* why ) {
	const char* call = updateCall( kind );
	const bool pose = ( kind == UpdateKind::Pose || kind == UpdateKind::PoseDQ );

	if( ( kind == UpdateKind::Morph || pose ) && f.numMorphTargets == 0 ) {
		return packFail( why, PBR_ESTATE, "%s without a morph: pbr_set_morph declares the targets and captures the rest pose (a new upload drops it)", call );
	}
	if( pose && f.numBones == 0 ) {
		return packFail( why, PBR_ESTATE, "%s without a skin: pbr_set_skin declares the influences (a new upload drops it)", call );
	}
	if( pose && f.skinGeneration != f.morphGeneration ) {
		return packFail( why, PBR_ESTATE, "%s: pbr_set_skin and pbr_set_morph captured different geometry (an upload or an update lies between them): set both on the same rest pose", call );
	}
	if( ( kind == UpdateKind::Skin || kind == UpdateKind::SkinDQ ) && f.numBones == 0 ) {
		return packFail( why, PBR_ESTATE, "%s without a skin: pbr_set_skin declares the influences and captures the rest pose (a new upload drops it)", call );
	}
	if( kind == UpdateKind::Transforms && f.numParts == 0 ) {
		return packFail( why, PBR_ESTATE, "pbr_update_transforms without parts: pbr_set_parts declares them and captures the rest pose (a new upload drops them)" );
	}
	if( ( kind == UpdateKind::Vertices || kind == UpdateKind::Geometry ) && !f.hasScene ) {
		return packFail( why, PBR_ESTATE, "%s before pbr_upload_scene", call );
	}

	return PBR_OK;
}

// a ray-ordered traversal is configured: its records carry child orders built from the boxes
inline bool updateOrdered( const UpdateFacts& f ) {
	return f.configured && f.traversal != 0;
}

// Stage 3.  bringsNormals: pbr_update_geometry was given new normals (no other kind brings any).
inline int admitShared( UpdateKind kind, bool bringsNormals, const UpdateFacts& f, std::string* why ) {
	const char* call = updateCall( kind );

	if( !f.nested ) {
		return packFail( why, PBR_ESTATE, "%s: the uploaded tree is not properly nested (%s); a refit needs the children of every container to tile its subtree", call, f.why );
	}
	if( updateOrdered( f ) && !f.refitOrdered ) {
		return packFail( why, PBR_ESTATE, "%s while a ray-ordered traversal (%u) is configured: its streams carry child orders built from the old boxes — configure traversal 0, update, then configure the ordered walk again", call, f.traversal );
	}
	if( kind == UpdateKind::Vertices && f.configured && f.phongTessellation > 0.0f ) {
		return packFail( why, PBR_ESTATE, "pbr_update_vertices while Phong tessellation is configured: tight boxes of the flat triangles would clip the patches" );
	}
	if( kind == UpdateKind::Geometry && bringsNormals && !f.hasPatches ) {
		return packFail( why, PBR_ESTATE, "pbr_update_geometry: new normals for a scene that was uploaded without usable vertex normals (its facesN / normals were missing or out of range, it has no Phong patches)" );
	}

	return PBR_OK;
}

// The kernel that writes N' behind the staged V' of a device kind.
enum class NormalKernel : uint32_t { None = 0, Transform, Skin, Morph, Pose, SkinDQ, PoseDQ };

// What an admitted call does.
struct UpdatePlan {
	bool ordered = false;       // updateOrdered: without a re-link the configured layout's records are rebuilt on the host
	bool gathers = false;       // the patches are gathered again: whenever the scene has any, for every kind but pbr_update_vertices
	float alpha = 0.0f;         // the boxes are thick ones for this phong_tessellation; 0: pbr_update_vertices's boxes, kernel for kernel
	bool relinks = false;       // pbr_refit_ordered_walk: the configured layout's records are re-linked in place behind the refit
	bool keepsHistory = false;  // pbr_denoise_temporal under motion tracking: H is copied before the vertices are replaced
	NormalKernel normals = NormalKernel::None;
};

inline UpdatePlan planUpdate( UpdateKind kind, const UpdateFacts& f ) {
	UpdatePlan plan;
	plan.ordered = updateOrdered( f );
	// Phong tessellation cannot be configured without patches
	plan.gathers = ( kind != UpdateKind::Vertices && f.hasPatches );
	plan.alpha = ( plan.gathers && f.configured && f.phongTessellation > 0.0f ) ? f.phongTessellation : 0.0f;
	plan.relinks = ( plan.ordered && f.walkBuilt );
	plan.keepsHistory = ( f.tracking && f.history && !f.moved );   // what TemporalPolicy::update() answers

	// the pose: morphed if the morph has normal targets, skinned if the skin has normal influences
	const bool dq = ( kind == UpdateKind::SkinDQ || kind == UpdateKind::PoseDQ );
	const bool morphs = ( ( kind == UpdateKind::Morph || kind == UpdateKind::Pose || kind == UpdateKind::PoseDQ ) && f.morphNormals );
	const bool skins = ( ( kind == UpdateKind::Skin || kind == UpdateKind::Pose || dq ) && f.skinNormals );

	if( kind == UpdateKind::Transforms && f.partNormals ) {
		plan.normals = NormalKernel::Transform;
	}
	else if( morphs ) {
		plan.normals = !skins ? NormalKernel::Morph : dq ? NormalKernel::PoseDQ : NormalKernel::Pose;
	}
	else if( skins ) {
		plan.normals = dq ? NormalKernel::SkinDQ : NormalKernel::Skin;
	}

	return plan;
}
