// dump.cpp — runs the reference's own host code (its loaders, its BVH builder, MathHelp::triCalcAABB), compiled unmodified
// by oracle/refhost.py, and writes what it produced as DATA: one flat binary file per run, read by oracle/refhost.py's
// read_dump.  TEST INFRASTRUCTURE ONLY: nothing here is part of the product, and nothing here computes a result.
//
//   refhost_dump scene <dir> <obj> out=<file> [key=value ...]    ModelLoader + BVH over <dir><obj>
//   refhost_dump faces <file> out=<file> alpha=<a> [key=value ...]   triCalcAABB over N hand-made faces
//
// key=value sets a Cfg key (the reference's Cfg has no file-less setter but value( key, void* ), which the ptree stand-in
// reads as text).  Defaults are config.json's: bvh.max_faces 2, bvh.sah_faces_limit 100000, bvh.skip_ahead true,
// bvh.skip_ahead_compare 0.7, render.phong_tessellation 0.0, render.shadow_rays 0; logging.level is 0 (config.json: 4) so a
// run prints nothing — no log line reaches the dump either way.
//
// File: records of { u32 name length, name, u8 type ('f' binary32, 'u' uint32, 'i' int32, 's' bytes), u32 dims, u32 dim[dims],
// payload }, little endian, in the order written.  Name lists are '\n'-joined bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "Cfg.h"
#include "MathHelp.h"
#include "ModelLoader.h"
#include "accelstructures/BVH.h"

using std::string;
using std::vector;

static const uint32_t NONE = 0xFFFFFFFFu;


struct Writer {
	FILE* f;

	void u32( uint32_t v ) { fwrite( &v, 4, 1, f ); }

	void record( const char* name, char type, const vector<uint32_t>& dims, const void* data, size_t bytes ) {
		u32( (uint32_t) strlen( name ) );
		fwrite( name, 1, strlen( name ), f );
		fwrite( &type, 1, 1, f );
		u32( (uint32_t) dims.size() );
		for( uint32_t d : dims ) { u32( d ); }
		if( bytes ) { fwrite( data, 1, bytes, f ); }
	}

	template<typename T> void array( const char* name, char type, const vector<T>& v, uint32_t columns ) {
		static_assert( sizeof( T ) == 4, "four-byte words only" );
		record( name, type, { (uint32_t) ( v.size() / columns ), columns }, v.data(), v.size() * 4 );
	}

	void text( const char* name, const string& s ) { record( name, 's', { (uint32_t) s.size() }, s.data(), s.size() ); }
};


static void setCfg( const char* key, const char* text ) { Cfg::get().value( key, (void*) text ); }


// Applies the defaults and the key=value arguments from argv[first] on; returns the out= path.
static string configure( int argc, char** argv, int first ) {
	setCfg( Cfg::BVH_MAXFACES, "2" );
	setCfg( Cfg::BVH_SAHFACESLIMIT, "100000" );
	setCfg( Cfg::BVH_SKIPAHEAD, "true" );
	setCfg( Cfg::BVH_SKIPAHEAD_CMP, "0.7" );
	setCfg( Cfg::RENDER_PHONGTESS, "0.0" );
	setCfg( Cfg::RENDER_SHADOWRAYS, "0" );
	setCfg( Cfg::LOG_LEVEL, "0" );

	string out;

	for( int i = first; i < argc; i++ ) {
		const char* eq = strchr( argv[i], '=' );

		if( !eq ) {
			fprintf( stderr, "refhost_dump: not key=value: %s\n", argv[i] );
			exit( 2 );
		}

		const string key( argv[i], eq - argv[i] );

		if( key == "out" ) { out = eq + 1; }
		else if( key == "alpha" ) { setCfg( Cfg::RENDER_PHONGTESS, eq + 1 ); }
		else { setCfg( key.c_str(), eq + 1 ); }
	}

	if( out.empty() ) {
		fprintf( stderr, "refhost_dump: out=<file> is required\n" );
		exit( 2 );
	}

	return out;
}


static void push3( vector<float>& v, const glm::vec3& a ) { v.push_back( a[0] ); v.push_back( a[1] ); v.push_back( a[2] ); }
static void push4( vector<float>& v, const cl_float4& a ) { v.push_back( a.x ); v.push_back( a.y ); v.push_back( a.z ); v.push_back( a.w ); }
static void push4( vector<uint32_t>& v, const cl_uint4& a ) { v.push_back( a.x ); v.push_back( a.y ); v.push_back( a.z ); v.push_back( a.w ); }


struct TreeDump {
	vector<uint32_t> nodes;      // id, depth, numSkipsToHere, skipNextLeft, parent id, left id, right id, number of faces
	vector<float> nodeBoxes;     // bbMin, bbMax
	vector<uint32_t> triFace, triNormals;
	vector<float> triBoxes;

	void visit( const BVHNode* node ) {   // depth first, left child first
		nodes.push_back( node->id );
		nodes.push_back( node->depth );
		nodes.push_back( node->numSkipsToHere );
		nodes.push_back( node->skipNextLeft ? 1u : 0u );
		nodes.push_back( node->parent ? node->parent->id : NONE );
		nodes.push_back( node->leftChild ? node->leftChild->id : NONE );
		nodes.push_back( node->rightChild ? node->rightChild->id : NONE );
		nodes.push_back( (uint32_t) node->faces.size() );
		push3( nodeBoxes, node->bbMin );
		push3( nodeBoxes, node->bbMax );

		for( const Tri& tri : node->faces ) {
			push4( triFace, tri.face );
			push4( triNormals, tri.normals );
			push3( triBoxes, tri.bbMin );
			push3( triBoxes, tri.bbMax );
		}

		if( node->leftChild ) { visit( node->leftChild ); }
		if( node->rightChild ) { visit( node->rightChild ); }
	}
};


static int dumpScene( const string& dir, const string& obj, const string& out ) {
	ModelLoader loader;
	loader.loadModel( dir, obj );
	ObjParser* op = loader.getObjParser();

	Writer w { fopen( out.c_str(), "wb" ) };
	if( !w.f ) { perror( out.c_str() ); return 1; }

	w.array( "vertices", 'f', op->getVertices(), 3 );
	w.array( "normals", 'f', op->getNormals(), 3 );
	w.array( "facesV", 'u', op->getFacesV(), 3 );
	w.array( "facesVN", 'u', op->getFacesVN(), 3 );
	w.array( "facesMtl", 'i', op->getFacesMtl(), 1 );

	const vector<object3D> objects = op->getObjects();
	string names;
	vector<uint32_t> ranges;      // per object: first face, number of faces, number of normal triples (running over the objects)
	uint32_t firstFace = 0;

	for( const object3D& o : objects ) {
		names += o.oName + "\n";
		ranges.push_back( firstFace );
		ranges.push_back( (uint32_t) ( o.facesV.size() / 3 ) );
		ranges.push_back( (uint32_t) ( o.facesVN.size() / 3 ) );
		firstFace += (uint32_t) ( o.facesV.size() / 3 );
	}

	w.text( "object_names", names );
	w.array( "object_ranges", 'u', ranges, 3 );

	names.clear();
	vector<float> mtlFloats;      // Ka, Kd, Ks (four words each), d, Ni, Ns, rough, p, nu, nv, Rs, Rd
	vector<int32_t> mtlInts;      // illum, light

	for( const material_t& m : op->getMaterials() ) {
		names += m.mtlName + "\n";
		push4( mtlFloats, m.Ka );
		push4( mtlFloats, m.Kd );
		push4( mtlFloats, m.Ks );
		const float rest[9] = { m.d, m.Ni, m.Ns, m.rough, m.p, m.nu, m.nv, m.Rs, m.Rd };
		mtlFloats.insert( mtlFloats.end(), rest, rest + 9 );
		mtlInts.push_back( m.illum );
		mtlInts.push_back( m.light );
	}

	w.text( "material_names", names );
	w.array( "material_floats", 'f', mtlFloats, 21 );
	w.array( "material_ints", 'i', mtlInts, 2 );

	names.clear();
	vector<float> lightFloats;    // pos, rgb (four words each), radius
	vector<uint32_t> lightTypes;

	for( const light_t& l : op->getLights() ) {
		names += l.lightName + "\n";
		push4( lightFloats, l.pos );
		push4( lightFloats, l.rgb );
		lightFloats.push_back( l.radius );
		lightTypes.push_back( l.type );
	}

	w.text( "light_names", names );
	w.array( "light_floats", 'f', lightFloats, 9 );
	w.array( "light_types", 'u', lightTypes, 1 );

	BVH bvh( objects, op->getVertices(), op->getNormals() );

	TreeDump tree;
	tree.visit( bvh.getRoot() );
	w.array( "tree_nodes", 'u', tree.nodes, 8 );
	w.array( "tree_boxes", 'f', tree.nodeBoxes, 6 );
	w.array( "tri_face", 'u', tree.triFace, 4 );
	w.array( "tri_normals", 'u', tree.triNormals, 4 );
	w.array( "tri_boxes", 'f', tree.triBoxes, 6 );

	// the builder's own node list, which PathTracer's flattening reads front to back: 1 if it is this depth-first order,
	// ids 0, 1, 2, ...
	const vector<BVHNode*> listed = bvh.getNodes();
	uint32_t inOrder = ( listed.size() * 8 == tree.nodes.size() ) ? 1u : 0u;

	for( size_t i = 0; inOrder && i < listed.size(); i++ ) {
		inOrder = ( listed[i]->id == i && tree.nodes[i * 8] == i ) ? 1u : 0u;
	}

	w.array( "nodes_in_id_order", 'u', vector<uint32_t>( 1, inOrder ), 1 );

	const vector<uint32_t> sizes = { (uint32_t) bvh.getNodes().size(), (uint32_t) bvh.getLeafNodes().size(), (uint32_t) bvh.getDepth() };
	w.array( "sizes", 'u', sizes, 3 );

	return fclose( w.f ) == 0 ? 0 : 1;
}


static int dumpFaces( const string& in, const string& out ) {
	FILE* f = fopen( in.c_str(), "rb" );
	if( !f ) { perror( in.c_str() ); return 1; }

	vector<float> words;          // per face: three corners, three normals, three words each
	float buffer[18];
	while( fread( buffer, 4, 18, f ) == 18 ) { words.insert( words.end(), buffer, buffer + 18 ); }
	fclose( f );

	const uint32_t count = (uint32_t) ( words.size() / 18 );
	vector<cl_float4> vertices4, normals4;

	for( uint32_t i = 0; i < count; i++ ) {
		for( uint32_t k = 0; k < 3; k++ ) {
			const float* p = &words[i * 18 + k * 3];
			const float* n = &words[i * 18 + 9 + k * 3];
			const cl_float4 p4 = { p[0], p[1], p[2], 0.0f }, n4 = { n[0], n[1], n[2], 0.0f };
			vertices4.push_back( p4 );
			normals4.push_back( n4 );
		}
	}

	vector<float> boxes;

	for( uint32_t i = 0; i < count; i++ ) {
		Tri tri;
		const cl_uint4 idx = { 3 * i, 3 * i + 1, 3 * i + 2, i };
		tri.face = idx;
		tri.normals = idx;
		MathHelp::triCalcAABB( &tri, &vertices4, &normals4 );   // as BVH::facesToTriStructs calls it
		push3( boxes, tri.bbMin );
		push3( boxes, tri.bbMax );
	}

	Writer w { fopen( out.c_str(), "wb" ) };
	if( !w.f ) { perror( out.c_str() ); return 1; }
	w.array( "boxes", 'f', boxes, 6 );
	return fclose( w.f ) == 0 ? 0 : 1;
}


int main( int argc, char** argv ) {
	if( argc >= 4 && string( argv[1] ) == "scene" ) {
		const string out = configure( argc, argv, 4 );
		return dumpScene( argv[2], argv[3], out );
	}

	if( argc >= 3 && string( argv[1] ) == "faces" ) {
		const string out = configure( argc, argv, 3 );
		return dumpFaces( argv[2], out );
	}

	fprintf( stderr, "usage: refhost_dump scene <dir> <obj> out=<file> [key=value ...]\n"
	                 "       refhost_dump faces <file> out=<file> alpha=<a> [key=value ...]\n" );
	return 2;
}
