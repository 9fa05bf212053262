// Exposes the host-only unit of pbr_set_parts / pbr_update_transforms (physically-based-rendering_amd/csrc/pt_transform_host.hpp —
// the very source the device kernels call per vertex and per normal) to tests/test_transform_cpu.py through ctypes: plain
// C++17, built with g++ -shared -ffp-contract=off like its sibling tests/patch_refit_driver.cpp.
//   tr_cofactors         per part: the nine cofactor words, the determinant before its sign was taken out, the identity test
//   tr_check_parts       what pbr_set_parts answers to these arrays before it touches the device
//   tr_check_transforms  what pbr_update_transforms answers to these matrices, and the 24-word records that travel
//   tr_transform         V' and N' of whole arrays from such records; returns the first position that is not finite, or -1
#include <cstdio>
#include <string>

#include "pt_transform_host.hpp"

extern "C" {

void tr_cofactors( const float* matrices, uint32_t num_parts, float* c_out, float* det_out, uint32_t* identity_out ) {
	for( uint32_t k = 0; k < num_parts; k++ ) {
		ptx::cofactors( matrices + (size_t) k * 12, c_out + (size_t) k * 9, det_out + k );
		identity_out[k] = ptx::isIdentity( matrices + (size_t) k * 12 ) ? 1u : 0u;
	}
}

int tr_check_parts( const uint32_t* vertex_part, uint32_t num_vertices, uint32_t uploaded_vertices, const uint32_t* normal_part, uint32_t num_normals,
                    uint32_t uploaded_normals, uint32_t num_parts, char* why, size_t capacity ) {
	std::string error;
	const int status = checkParts( vertex_part, num_vertices, uploaded_vertices, normal_part, num_normals, uploaded_normals, num_parts, &error );
	std::snprintf( why, capacity, "%s", error.c_str() );
	return status;
}

int tr_check_transforms( const float* matrices, uint32_t num_parts, uint32_t set_parts, void* records_out, char* why, size_t capacity ) {
	std::string error;
	const int status = checkTransforms( matrices, num_parts, set_parts, (ptx::PartRecord*) records_out, &error );
	std::snprintf( why, capacity, "%s", error.c_str() );
	return status;
}

long long tr_transform( const void* records, const pbr_float4* rest, const uint32_t* vertex_part, uint32_t num_vertices, pbr_float4* vertices_out,
                        const pbr_float4* rest_normals, const uint32_t* normal_part, uint32_t num_normals, pbr_float4* normals_out ) {
	return transformArrays( (const ptx::PartRecord*) records, rest, vertex_part, num_vertices, vertices_out, rest_normals, normal_part, num_normals, normals_out );
}

}  // extern "C"
