// Drives the schedule tuner (physically-based-rendering_amd/csrc/pt_tuner.hpp) the way launch() does, with synthetic timings:
// a chunk of n frames of plan p takes ( a[p] + b[p] x n ) x the next noise factor ms, as a float (hipEventElapsedTime's type).
// The scenario file (tests/test_schedule_tuner_cpu.py):
//   scale S              the tuner's scale (ScheduleTuner::scaleOf)
//   log                  print the tuner's [pbr tune] lines too
//   cap C                at most C frames per chunk (the frame buffer's cap / the chunk_frames knob)
//   cost a0 b0 ... a6 b6 per plan, ms
//   noise f0 f1 ...      per launch, cycled
//   calls n0 n1 ...      the render calls' lengths
// Prints the budget, then per call its chunks (plan:frames, then "s" screening / "f<k>" finalist k) and the decision, and at
// the end every plan's fit.
#include <cstdio>
#include <string>
#include <vector>

#include "pt_tuner.hpp"

int main( int argc, char** argv ) {
	FILE* in = ( argc == 2 ) ? std::fopen( argv[1], "r" ) : nullptr;

	if( in == nullptr ) {
		return 2;
	}

	const int kPlans = ScheduleTuner::kPlans;
	const char* const names[kPlans] = { "refill-lean", "refill-wide", "phased-lean", "phased-wide", "phased-mid", "refill-mid", "phased-dual" };
	double costA[kPlans] = {}, costB[kPlans] = {};
	std::vector<double> noise;
	std::vector<uint32_t> calls;
	unsigned scale = 1, cap = 0xFFFFFFFFu;
	bool log = false;
	char word[32];

	while( std::fscanf( in, "%31s", word ) == 1 ) {
		const std::string w = word;
		bool ok = true;

		if( w == "scale" ) {
			ok = std::fscanf( in, "%u", &scale ) == 1;
		}
		else if( w == "log" ) {
			log = true;
		}
		else if( w == "cap" ) {
			ok = std::fscanf( in, "%u", &cap ) == 1;
		}
		else if( w == "cost" ) {
			for( int k = 0; k < kPlans && ok; k++ ) {
				ok = std::fscanf( in, "%lf %lf", &costA[k], &costB[k] ) == 2;
			}
		}
		else if( w == "noise" ) {
			for( double f; std::fscanf( in, "%lf", &f ) == 1; ) {
				noise.push_back( f );
			}
		}
		else if( w == "calls" ) {
			for( unsigned n; std::fscanf( in, "%u", &n ) == 1; ) {
				calls.push_back( n );
			}
		}
		else {
			ok = false;
		}

		if( !ok ) {
			std::fprintf( stderr, "bad scenario at '%s'\n", word );
			return 2;
		}

		std::clearerr( in );
	}

	std::fclose( in );

	if( noise.empty() ) {
		noise.push_back( 1.0 );
	}

	ScheduleTuner tuner;
	tuner.reset( scale );
	tuner.log = log ? stdout : nullptr;

	for( int k = 0; k < kPlans; k++ ) {
		tuner.names[k] = names[k];
	}

	std::printf( "budget %u\n", tuner.budgetFrames() );
	size_t launches = 0;

	for( const uint32_t nFrames : calls ) {
		tuner.beginRender( nFrames );
		std::printf( "call %u:", nFrames );

		for( uint32_t done = 0; done < nFrames; ) {
			const Chunk chunk = tuner.next( std::min<uint32_t>( cap, nFrames - done ) );
			const float ms = (float) ( ( costA[chunk.plan] + costB[chunk.plan] * (double) chunk.frames ) * noise[launches++ % noise.size()] );
			std::printf( " %d:%u%s", chunk.plan, chunk.frames, chunk.screening ? "s" : ( chunk.finalist >= 0 ) ? ( "f" + std::to_string( chunk.finalist ) ).c_str() : "" );

			if( log && ( chunk.screening || chunk.finalist >= 0 ) ) {
				std::printf( "\n" );
			}

			tuner.record( chunk, (double) ms );
			done += chunk.frames;
		}

		std::printf( "\n  -> %d%s\n", tuner.tunedPlan(), tuner.settled() ? "" : " (measuring)" );
	}

	for( int k = 0; k < kPlans; k++ ) {
		double a, b;

		if( tuner.fit( k, &a, &b ) ) {
			std::printf( "fit %d: %.6f %.6f\n", k, a, b );
		}
		else {
			std::printf( "fit %d: none\n", k );
		}
	}

	return 0;
}
