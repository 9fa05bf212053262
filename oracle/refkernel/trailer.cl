/*
 * trailer.cl — appended to the reference's assembled kernel text by oracle/refkernel.py (own text, OpenCL C): it only
 * CALLS the reference's functions by name, with every argument behind a pointer so that the driver needs to know no
 * by-value vector or struct ABI.  TEST INFRASTRUCTURE ONLY.
 */

/* the compile-time values of this binary, for the driver to check its inputs against */
int rk_const( int which ) {
	switch( which ) {
		case 0: return IMG_WIDTH;
		case 1: return IMG_HEIGHT;
		case 2: return BRDF;
		case 3: return BVH_NUM_NODES;
		case 4: return NUM_LIGHTS;
		case 5: return (int) sizeof( material );
		case 6: return (int) sizeof( camera );
		case 7: return (int) sizeof( bvhNode );
		case 8: return (int) sizeof( light_t );
		case 9: return PHONGTESS;
	}
	return -1;
}

/* one work item of the kernel; get_global_id is the driver's */
void rk_pixel(
	float seed, float pixelWeight, float pxDim, global const camera* cam,
	global const bvhNode* bvh, global const uint4* facesV, global const uint4* facesN, global const float4* vertices,
	global const float4* normals, global const material* materials, global const light_t* lights,
	read_only image2d_t imageIn, write_only image2d_t imageOut, write_only image2d_t imageDebug
) {
	pathTracing( seed, pixelWeight, pxDim, *cam, bvh, facesV, facesN, vertices, normals, materials, lights, imageIn, imageOut, imageDebug );
}

/* closest hit of one ray: out = { t, hitFace, normal.xyz, node visits, face tests }; *t0 is what ray.t starts from */
void rk_ray(
	global const bvhNode* bvh, global const uint4* facesV, global const uint4* facesN, global const float4* vertices,
	global const float4* normals, global const light_t* lights, global const float* ray6, global const float* t0,
	global float* out7, global int* outFace
) {
	Scene scene = { bvh, lights, facesV, facesN, vertices, normals, (float4)( 0.0f ) };
	ray4 ray;
	ray.origin = (float3)( ray6[0], ray6[1], ray6[2] );
	ray.dir = (float3)( ray6[3], ray6[4], ray6[5] );
	ray.normal = (float3)( 0.0f );
	ray.t = *t0;
	ray.hitFace = 0;

	traverse( &scene, &ray );

	out7[0] = ray.t;
	out7[1] = ray.normal.x;
	out7[2] = ray.normal.y;
	out7[3] = ray.normal.z;
	out7[4] = scene.debugColor.y;
	out7[5] = scene.debugColor.x;
	*outFace = ray.hitFace;
}

/* the shadow walk of one ray, ray7 = { origin, dir, tLight }: out = { t, face tests } as traverseShadows leaves the ray
 * (intersectFace counts its tests in debugColor.x in both walks; the shadow walk counts no node visits) */
void rk_shadow_ray(
	global const bvhNode* bvh, global const uint4* facesV, global const uint4* facesN, global const float4* vertices,
	global const float4* normals, global const light_t* lights, global const float* ray7, global float* out2, global int* outFace
) {
	Scene scene = { bvh, lights, facesV, facesN, vertices, normals, (float4)( 0.0f ) };
	ray4 ray;
	ray.origin = (float3)( ray7[0], ray7[1], ray7[2] );
	ray.dir = (float3)( ray7[3], ray7[4], ray7[5] );
	ray.normal = (float3)( 0.0f );
	ray.t = ray7[6];
	ray.hitFace = 0;

	traverseShadows( &scene, &ray );

	out2[0] = ray.t;
	out2[1] = scene.debugColor.x;
	*outFace = ray.hitFace;
}
