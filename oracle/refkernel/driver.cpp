/*
 * driver.cpp — data-only driver of the compiled reference kernel (oracle/refkernel.py).  TEST INFRASTRUCTURE ONLY, own text.
 *
 *     refkernel_<key> in=<records> out=<records>
 *
 * Records, as oracle/refhost/dump.cpp writes them: u32 name length, name, kind ('f' float32, 'u' uint32, 'i' int32),
 * u32 rank, u32 dims[rank], data.  Read: the seven wire arrays (bvh, facesV, facesN, vertices, normals, materials,
 * lights), camera (20 words), seeds, first (the first sample count), px_dim, rays (n x 6, may be empty).  Written:
 * image, debug (H x W x 4), frame_counts (frames x {node visits, face tests}: the sums of each frame's debug image), ray_t, ray_face, ray_normal, ray_counts {node visits, face tests}.
 * Optional: t0 (one value per ray of `rays`: what its t starts from, +inf without the record) and shadow_rays (n x 7:
 * origin, dir, tLight) — with the latter shadow_t, shadow_face, shadow_tests are written too: each ray as the reference's
 * traverseShadows leaves it, and its face tests.
 *
 * Frames follow the reference's host loop: the last output becomes the next input, the weight of frame n is
 * n / ( n + 1 ) in float32, the debug image is the last frame's.  Every index the kernel is handed is checked against the
 * arrays first, and the arrays against the values compiled into this binary.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

struct rk_image {
	float* texels;
	int width, height;
};

extern "C" {
int rk_const( int which );
void rk_set_global_id( unsigned long x, unsigned long y );
void rk_pixel(
	float seed, float pixelWeight, float pxDim, const void* cam,
	const void* bvh, const void* facesV, const void* facesN, const void* vertices, const void* normals,
	const void* materials, const void* lights, rk_image* imageIn, rk_image* imageOut, rk_image* imageDebug );
void rk_ray(
	const void* bvh, const void* facesV, const void* facesN, const void* vertices, const void* normals,
	const void* lights, const float* ray6, const float* t0, float* out7, int32_t* outFace );
void rk_shadow_ray(
	const void* bvh, const void* facesV, const void* facesN, const void* vertices, const void* normals,
	const void* lights, const float* ray7, float* out2, int32_t* outFace );
}

struct Record {
	char kind;
	std::vector<uint32_t> dims;
	std::vector<uint32_t> words;
	size_t rows() const { return dims.empty() ? 0 : dims[0]; }
	size_t cols() const { return dims.size() < 2 ? 1 : dims[1]; }
};

static void fail( const std::string& what ) {
	fprintf( stderr, "refkernel: %s\n", what.c_str() );
	exit( 2 );
}

static std::map<std::string, Record> readRecords( const char* path ) {
	FILE* f = fopen( path, "rb" );
	if( !f ) fail( std::string( "cannot open " ) + path );
	std::map<std::string, Record> out;
	uint32_t n;
	while( fread( &n, 4, 1, f ) == 1 ) {
		if( n > 256 ) fail( "bad record name" );
		std::string name( n, '\0' );
		Record r;
		uint32_t rank;
		if( fread( &name[0], 1, n, f ) != n || fread( &r.kind, 1, 1, f ) != 1 || fread( &rank, 4, 1, f ) != 1 || rank > 4 ) fail( "bad record header" );
		r.dims.resize( rank );
		size_t count = 1;
		for( uint32_t k = 0; k < rank; k++ ) {
			if( fread( &r.dims[k], 4, 1, f ) != 1 ) fail( "bad record dims" );
			count *= r.dims[k];
		}
		if( count > ( 1u << 28 ) ) fail( "record too large" );
		r.words.resize( count );
		if( count && fread( r.words.data(), 4, count, f ) != count ) fail( "short record " + name );
		out[name] = r;
	}
	fclose( f );
	return out;
}

static void writeRecord( FILE* f, const char* name, char kind, std::vector<uint32_t> dims, const void* data ) {
	uint32_t n = (uint32_t) strlen( name ), rank = (uint32_t) dims.size();
	size_t count = 1;
	for( uint32_t d : dims ) count *= d;
	fwrite( &n, 4, 1, f );
	fwrite( name, 1, n, f );
	fwrite( &kind, 1, 1, f );
	fwrite( &rank, 4, 1, f );
	fwrite( dims.data(), 4, rank, f );
	if( count ) fwrite( data, 4, count, f );
}

static const Record& need( const std::map<std::string, Record>& in, const char* name, char kind, size_t cols ) {
	auto it = in.find( name );
	if( it == in.end() ) fail( std::string( "missing record " ) + name );
	if( it->second.kind != kind || ( it->second.rows() && it->second.cols() != cols ) ) fail( std::string( "bad shape or type: " ) + name );
	return it->second;
}

int main( int argc, char** argv ) {
	const char *inPath = nullptr, *outPath = nullptr;
	for( int i = 1; i < argc; i++ ) {
		if( !strncmp( argv[i], "in=", 3 ) ) inPath = argv[i] + 3;
		if( !strncmp( argv[i], "out=", 4 ) ) outPath = argv[i] + 4;
	}
	if( !inPath || !outPath ) fail( "usage: in=<records> out=<records>" );

	const int W = rk_const( 0 ), H = rk_const( 1 ), brdf = rk_const( 2 ), numNodes = rk_const( 3 ), numLights = rk_const( 4 );
	if( rk_const( 5 ) != ( brdf == 0 ? 48 : 64 ) || rk_const( 6 ) != 80 || rk_const( 7 ) != 32 || rk_const( 8 ) != 48 ) fail( "struct layouts differ from the wire formats" );

	const auto in = readRecords( inPath );
	const Record& bvh = need( in, "bvh", 'f', 8 );
	const Record& facesV = need( in, "facesV", 'u', 4 );
	const Record& facesN = need( in, "facesN", 'u', 4 );
	const Record& vertices = need( in, "vertices", 'f', 4 );
	const Record& normals = need( in, "normals", 'f', 4 );
	const Record& materials = need( in, "materials", 'f', brdf == 0 ? 12 : 16 );
	const Record& lights = need( in, "lights", 'f', 12 );
	const Record& camera = need( in, "camera", 'u', 1 );
	const Record& seeds = need( in, "seeds", 'f', 1 );
	const Record& first = need( in, "first", 'u', 1 );
	const Record& pxDim = need( in, "px_dim", 'f', 1 );
	const Record& rays = need( in, "rays", 'f', 6 );
	const Record* t0 = in.count( "t0" ) ? &need( in, "t0", 'f', 1 ) : nullptr;
	const Record* shadowRays = in.count( "shadow_rays" ) ? &need( in, "shadow_rays", 'f', 7 ) : nullptr;
	if( t0 && t0->words.size() != rays.rows() ) fail( "t0 does not fit rays" );

	if( (int) bvh.rows() != numNodes || (int) lights.rows() != numLights ) fail( "node or light count differs from the compiled one" );
	if( numNodes < 2 || camera.words.size() != 20 || first.words.size() != 1 || pxDim.words.size() != 1 ) fail( "bad scalar records" );
	const bool phong = rk_const( 9 ) != 0;          /* facesN and normals are read only then */
	if( ( phong && facesN.rows() != facesV.rows() ) || !materials.rows() ) fail( "facesN / materials do not fit facesV" );
	for( size_t k = 0; k < facesV.rows(); k++ ) {
		const uint32_t* v = &facesV.words[4 * k];
		const uint32_t* nn = phong ? &facesN.words[4 * k] : v;
		if( v[0] >= vertices.rows() || v[1] >= vertices.rows() || v[2] >= vertices.rows() || v[3] >= materials.rows() ) fail( "facesV out of range" );
		if( phong && ( nn[0] >= normals.rows() || nn[1] >= normals.rows() || nn[2] >= normals.rows() ) ) fail( "facesN out of range" );
	}
	for( size_t k = 0; k < bvh.rows(); k++ ) {          /* leaves name faces; inner nodes name the next node, which the walk itself bounds */
		float lo, hi;
		memcpy( &lo, &bvh.words[8 * k + 3], 4 );
		memcpy( &hi, &bvh.words[8 * k + 7], 4 );
		if( lo >= 0.0f && ( !( lo < (float) facesV.rows() ) || ( hi != -1.0f && !( hi >= 0.0f && hi < (float) facesV.rows() ) ) ) ) fail( "leaf names a face out of range" );
	}

	/* the kernel's structs ask for up to 32-byte alignment (float8) */
	auto aligned = []( const Record& r ) -> const uint32_t* {
		void* p = aligned_alloc( 64, ( r.words.size() * 4 + 127 ) / 64 * 64 );
		if( !p ) fail( "out of memory" );
		memcpy( p, r.words.data(), r.words.size() * 4 );
		return (const uint32_t*) p;
	};
	const uint32_t *dCam = aligned( camera ), *dBvh = aligned( bvh ), *dFacesV = aligned( facesV ), *dFacesN = aligned( facesN ),
		*dVertices = aligned( vertices ), *dNormals = aligned( normals ), *dMaterials = aligned( materials ), *dLights = aligned( lights );

	std::vector<float> imgA( (size_t) W * H * 4, 0.0f ), imgB( imgA ), dbg( imgA );
	uint32_t n = first.words[0];
	std::vector<uint32_t> frameCounts;
	float px;
	memcpy( &px, &pxDim.words[0], 4 );

	for( size_t k = 0; k < seeds.words.size(); k++, n++ ) {
		float seed;
		memcpy( &seed, &seeds.words[k], 4 );
		const float weight = (float) n / (float) ( n + 1 );
		imgA = imgB;
		rk_image imageIn = { imgA.data(), W, H }, imageOut = { imgB.data(), W, H }, imageDebug = { dbg.data(), W, H };
		for( int y = 0; y < H; y++ ) {
			for( int x = 0; x < W; x++ ) {
				rk_set_global_id( (unsigned long) x, (unsigned long) y );
				rk_pixel( seed, weight, px, dCam, dBvh, dFacesV, dFacesN, dVertices, dNormals, dMaterials, dLights, &imageIn, &imageOut, &imageDebug );
			}
		}
		/* this frame's debug image as counts: the kernel divides face tests by 1082 and node visits by 1265 */
		uint64_t nodes = 0, tris = 0;
		for( size_t p = 0; p < (size_t) W * H; p++ ) {
			tris += (uint64_t) llrint( (double) dbg[4 * p + 0] * 1082.0 );
			nodes += (uint64_t) llrint( (double) dbg[4 * p + 1] * 1265.0 );
		}
		frameCounts.push_back( (uint32_t) nodes );
		frameCounts.push_back( (uint32_t) tris );
	}

	const uint32_t nr = (uint32_t) rays.rows();
	std::vector<float> rayT( nr ), rayNormal( 3 * (size_t) nr );
	std::vector<int32_t> rayFace( nr );
	std::vector<uint32_t> rayCounts( 2 * (size_t) nr );
	for( uint32_t k = 0; k < nr; k++ ) {
		float out7[7] = { 0 };
		const float inf = INFINITY;
		rk_ray( dBvh, dFacesV, dFacesN, dVertices, dNormals, dLights, (const float*) &rays.words[6 * (size_t) k],
		        t0 ? (const float*) &t0->words[k] : &inf, out7, &rayFace[k] );
		rayT[k] = out7[0];
		memcpy( &rayNormal[3 * (size_t) k], out7 + 1, 12 );
		rayCounts[2 * (size_t) k] = (uint32_t) out7[4];
		rayCounts[2 * (size_t) k + 1] = (uint32_t) out7[5];
	}

	const uint32_t ns = shadowRays ? (uint32_t) shadowRays->rows() : 0;
	std::vector<float> shadowT( ns );
	std::vector<int32_t> shadowFace( ns );
	std::vector<uint32_t> shadowTests( ns );
	for( uint32_t k = 0; k < ns; k++ ) {
		float out2[2] = { 0 };
		rk_shadow_ray( dBvh, dFacesV, dFacesN, dVertices, dNormals, dLights, (const float*) &shadowRays->words[7 * (size_t) k], out2, &shadowFace[k] );
		shadowT[k] = out2[0];
		shadowTests[k] = (uint32_t) out2[1];
	}

	FILE* f = fopen( outPath, "wb" );
	if( !f ) fail( std::string( "cannot write " ) + outPath );
	writeRecord( f, "image", 'f', { (uint32_t) H, (uint32_t) W, 4 }, imgB.data() );
	writeRecord( f, "debug", 'f', { (uint32_t) H, (uint32_t) W, 4 }, dbg.data() );
	writeRecord( f, "frame_counts", 'u', { (uint32_t) seeds.words.size(), 2 }, frameCounts.data() );
	writeRecord( f, "ray_t", 'f', { nr }, rayT.data() );
	writeRecord( f, "ray_face", 'i', { nr }, rayFace.data() );
	writeRecord( f, "ray_normal", 'f', { nr, 3 }, rayNormal.data() );
	writeRecord( f, "ray_counts", 'u', { nr, 2 }, rayCounts.data() );
	if( shadowRays ) {
		writeRecord( f, "shadow_t", 'f', { ns }, shadowT.data() );
		writeRecord( f, "shadow_face", 'i', { ns }, shadowFace.data() );
		writeRecord( f, "shadow_tests", 'u', { ns }, shadowTests.data() );
	}
	fclose( f );
	return 0;
}
