// Render driver: the host half of the hot path.  Mirrors the reference's PathTracer
// (source/PathTracer.h:80-146) and the part of Camera it reads (source/Camera.h,
// Camera.cpp:80-107) with the same method names, but talks to the HIP core through the C ABI
// (include/pbr_hip.h) instead of `CL`, and keeps the accumulated image on the device.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "bvh_builder.h"
#include "model_io.h"
#include "pbr_hip.h"

namespace pbr {

// The flat arrays PathTracer::initOpenCLBuffers_* upload (PathTracer.cpp:238-533), in the
// reference's wire formats.  Pure host data: built and testable without a device.
struct SceneBuffers {
	std::vector<pbr_bvh_node> bvh;
	std::vector<pbr_uint4> facesV;
	std::vector<pbr_uint4> facesN;
	std::vector<pbr_float4> vertices;
	std::vector<pbr_float4> normals;
	std::vector<pbr_material_schlick> materialsSchlick;  // filled when brdf == 0
	std::vector<pbr_material_sa> materialsSA;            // filled when brdf == 1
	std::vector<pbr_light> lights;                       // >= 1 entry (dummy when the scene has none)
	uint32_t numLights = 0;                              // #NUM_LIGHTS#
	uint32_t brdf = 1;
	float skyLight[4] = { 1.0f, 1.0f, 1.0f, 0.0f };      // #SKY_LIGHT#

	// initOpenCLBuffers_Faces / _BVH / _Materials / _Lights in the reference's order
	// (PathTracer.cpp:164-210).  Reads render.brdf from Cfg.
	void build( ModelLoader* ml, BVH* bvh );
	pbr_scene_desc desc() const;
};


// camera_t subset + Camera::cameraReset / getAdjustedCenter_glmVec3 (Camera.cpp:80-107).
class Camera {

	public:
		Camera();
		void cameraReset();
		void setEye( float x, float y, float z ) { mEye[0] = x; mEye[1] = y; mEye[2] = z; }
		// `center` is a view direction in the reference's convention: target = eye + (cx, -cy, -cz).
		void setCenter( float x, float y, float z );
		void getAdjustedCenter( float out[3] ) const;
		const float* getEye() const { return mEye; }
		const float* getUp() const { return mUp; }

	private:
		float mEye[3], mCenter[3], mUp[3];

};


class PathTracer {

	public:
		// `device`: HIP device ordinal for the context created in initOpenCLBuffers.
		explicit PathTracer( int device = 0 );
		~PathTracer();

		// PathTracer::initOpenCLBuffers (PathTracer.cpp:136-230): new context, upload, configure.
		// Throws std::runtime_error with the C ABI's message on failure (the reference exit()s).
		void initOpenCLBuffers(
			std::vector<float> vertices, std::vector<uint32_t> faces, std::vector<float> normals,
			ModelLoader* ml, AccelStructure* bvh
		);
		// PathTracer::generateImage (PathTracer.cpp:59-71): one frame; returns the accumulated image,
		// fills *textureDebug.  The seed is the fixed sequence seedStep * (n + 1) instead of the
		// wall clock (:63,78-82) so that renders are reproducible.
		std::vector<float> generateImage( std::vector<float>* textureDebug );
		// `frames` x generateImage in one device launch (no per-frame host round trip).
		std::vector<float> generateImages( uint32_t frames );
		// generateImages with adaptive sampling (pbr_render_adaptive): minFrames for every 8x8 tile, then roundFrames at a time
		// for the tiles whose error estimate is above `threshold`, maxFrames at most.  A NEW accumulation (sample count 0), and
		// the sample count is 0 again afterwards: the image then has a count per tile, which no later frame can continue.
		// Needs a camera without a focus point (setFocus): depth of field reads the focus pixel's every frame.
		std::vector<float> generateImagesAdaptive( uint32_t minFrames, uint32_t roundFrames, uint32_t maxFrames, float threshold );

		// pbr_update_vertices: new positions for the scene's vertices (count as uploaded), the BVH refitted on the device; starts
		// a new accumulation.  The host copy of the scene (buffers()) keeps the uploaded vertices and boxes.
		void updateVertices( const pbr_float4* vertices, uint32_t numVertices );
		// pbr_update_geometry: new positions and, unless null, new vertex normals (counts as uploaded): what updateVertices
		// rebuilds plus the Phong patches, with boxes thick enough for the configured render.phong_tessellation — the update
		// that works while Phong tessellation is on; starts a new accumulation
		void updateGeometry( const pbr_float4* vertices, uint32_t numVertices, const pbr_float4* normals, uint32_t numNormals );
		// pbr_set_parts: the part of every vertex and (unless null) of every vertex normal; captures the rest pose the
		// transforms start from
		void setParts( const uint32_t* vertexPart, uint32_t numVertices, const uint32_t* normalPart, uint32_t numNormals, uint32_t numParts );
		// pbr_update_transforms: one row-major 3 x 4 matrix per part; positions and normals are computed on the device from
		// the rest pose, then everything updateGeometry rebuilds; starts a new accumulation
		void updateTransforms( const float* matrices, uint32_t numParts );
		// pbr_set_skin: four bones and four weights for every vertex and (unless null) for every vertex normal; captures the
		// rest pose the skin updates start from
		void setSkin( const uint32_t* vertexBones, const float* vertexWeights, uint32_t numVertices, const uint32_t* normalBones, const float* normalWeights,
		              uint32_t numNormals, uint32_t numBones );
		// pbr_update_skin: one row-major 3 x 4 matrix per bone; positions and normals are blended on the device from the rest
		// pose, then everything updateGeometry rebuilds; starts a new accumulation
		void updateSkin( const float* matrices, uint32_t numBones );
		// pbr_set_morph: sparse morph targets, target-major, for the vertices and (unless null) for the vertex normals; captures
		// the rest pose the morph and pose updates start from
		void setMorph( const uint32_t* vertexFirst, const uint32_t* vertexIndex, const pbr_float4* vertexDelta, const uint32_t* normalFirst,
		               const uint32_t* normalIndex, const pbr_float4* normalDelta, uint32_t numTargets );
		// pbr_update_morph: one weight per target; positions and normals are morphed on the device from the rest pose, then
		// everything updateGeometry rebuilds; starts a new accumulation
		void updateMorph( const float* weights, uint32_t numTargets );
		// pbr_update_pose: the skin of the morphed rest pose — the weights and one row-major 3 x 4 matrix per bone
		void updatePose( const float* weights, uint32_t numTargets, const float* matrices, uint32_t numBones );
		// pbr_update_skin_dq: one dual quaternion (eight floats) per bone of the skin setSkin set; starts a new accumulation
		void updateSkinDQ( const float* dualQuats, uint32_t numBones );
		// pbr_update_pose_dq: the dual-quaternion skin of the morphed rest pose — the weights and one dual quaternion per bone
		void updatePoseDQ( const float* weights, uint32_t numTargets, const float* dualQuats, uint32_t numBones );
		// pbr_refit_ordered_walk: while on, updateVertices works under a ray-ordered traversal (the records are re-linked on the device)
		void refitOrderedWalk( bool on );

		void resetSampleCount();
		void setCamera( Camera* camera ) { mCamera = camera; }
		void setFocus( int x, int y );
		void setFOV( float fov ) { mFOV = fov; }
		void setWidthAndHeight( uint32_t width, uint32_t height ) { mWidth = width; mHeight = height; }
		void setSeedStep( float step ) { mSeedStep = step; }
		void setTiles( uint32_t world, uint32_t rank ) { mTileWorld = world; mTileRank = rank; }

		uint32_t getSampleCount() const { return mSampleCount; }
		double getKernelTime() const;
		pbr_ctx* context() { return mCtx; }
		const SceneBuffers& buffers() const { return mBuffers; }
		const pbr_camera& camera() const { return mStructCam; }

		// initKernelArgs' pixel size (PathTracer.cpp:89-91)
		static float pixelDimension( uint32_t width, uint32_t height, float fovDegrees );
		// updateEyeBuffer (PathTracer.cpp:628-652)
		static void fillCameraBasis( const Camera& cam, pbr_camera* out );
		// The pbr_config the current Cfg + buffers imply (CL::setValues, CL.cpp:626-705)
		static pbr_config makeConfig( const SceneBuffers& buffers, uint32_t width, uint32_t height );

	private:
		void updateEyeBuffer();
		void check( int status, const char* what );

		int mDevice;
		uint32_t mWidth, mHeight;
		float mFOV;
		uint32_t mSampleCount;
		float mSeedStep;
		uint32_t mTileWorld, mTileRank;
		pbr_camera mStructCam;
		Camera* mCamera;
		pbr_ctx* mCtx;
		SceneBuffers mBuffers;

};

}  // namespace pbr
