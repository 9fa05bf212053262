// pt_adaptive_host.hpp — the host side of pbr_render_adaptive (pbr_hip.hip, launchAdaptive) that needs no device: what the
// call refuses and how its frames fall into rounds and launch pairs (the dealing table of a round that renders only the tiles
// that are still active: pt_deal.hpp, filterOrder).  Host code only, no HIP: tests/adaptive_driver.cpp builds it with a plain
// C++17 compiler.
//
// An adaptive render runs in ROUNDS.  Round 0 renders frames [0, min_frames) of every local tile; every later round the next
// min( round_frames, max_frames - done ) frames of the tiles that have not stopped.  A tile's convergence is tested at round
// ends only (csrc/pt_adaptive.hpp), a tile that stopped never comes back, so all active tiles always hold the same number of
// frames.  Inside a round the frames are cut into launch pairs (path tracing + fold) of at most `chunkCap` frames — the
// frame buffer's cap, as in launch().
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "pbr_hip.h"
#include "pt_deal.hpp"   // filterOrder: a round's dealing table; whoever drives an adaptive render needs both

// Why pbr_render_adaptive refuses these arguments (PBR_EINVAL, the message in *why), or PBR_OK.
inline int adaptiveCheck( const pbr_adaptive_params* params, const float* seeds, const pbr_camera* cam, std::string* why ) {
	char buf[256];

	if( params == nullptr || seeds == nullptr || cam == nullptr ) {
		*why = "pbr_render_adaptive: null camera / seeds / params";
		return PBR_EINVAL;
	}
	if( cam->focusPoint[0] >= 0 && cam->focusPoint[1] >= 0 ) {
		*why = "pbr_render_adaptive needs focusPoint < 0: every pixel reads the focus pixel's previous frame, and the focus pixel's tile may stop; render depth of field with pbr_render_dof";
		return PBR_EINVAL;
	}
	if( params->min_frames < 2u ) {
		std::snprintf( buf, sizeof( buf ), "pbr_render_adaptive: min_frames %u < 2 (a variance needs two frames)", params->min_frames );
		*why = buf;
		return PBR_EINVAL;
	}
	if( params->max_frames < params->min_frames ) {
		std::snprintf( buf, sizeof( buf ), "pbr_render_adaptive: max_frames %u < min_frames %u", params->max_frames, params->min_frames );
		*why = buf;
		return PBR_EINVAL;
	}
	if( params->round_frames < 1u ) {
		*why = "pbr_render_adaptive: round_frames 0 (a round renders at least one frame)";
		return PBR_EINVAL;
	}
	if( std::isnan( params->threshold ) || params->threshold < 0.0f ) {
		std::snprintf( buf, sizeof( buf ), "pbr_render_adaptive: threshold %g is negative or not a number (0: only constant tiles stop, +inf: all stop at min_frames)", (double) params->threshold );
		*why = buf;
		return PBR_EINVAL;
	}

	return PBR_OK;
}

// One launch pair of an adaptive render: frames [first, first + frames) of the call; endsRound: the tiles are tested behind it.
struct AdaptivePair {
	uint32_t first, frames;
	bool endsRound;
};

// The launch pairs of a call IF no tile stops (a call ends early when none is active): rounds of min_frames, then round_frames
// — the last one shorter if they do not divide the rest —, each cut into pairs of at most chunkCap frames.
inline std::vector<AdaptivePair> adaptiveSchedule( uint32_t minFrames, uint32_t roundFrames, uint32_t maxFrames, uint32_t chunkCap ) {
	std::vector<AdaptivePair> pairs;
	chunkCap = ( chunkCap < 1u ) ? 1u : chunkCap;

	for( uint32_t done = 0; done < maxFrames; ) {
		const uint32_t round = ( done == 0u ) ? minFrames : ( roundFrames < maxFrames - done ? roundFrames : maxFrames - done );

		for( uint32_t at = 0; at < round; ) {
			const uint32_t n = ( chunkCap < round - at ) ? chunkCap : round - at;
			pairs.push_back( AdaptivePair{ done + at, n, at + n == round } );
			at += n;
		}

		done += round;
	}

	return pairs;
}

inline uint32_t adaptiveRounds( const std::vector<AdaptivePair>& pairs ) {
	uint32_t rounds = 0;

	for( const AdaptivePair& p : pairs ) {
		rounds += p.endsRound ? 1u : 0u;
	}

	return rounds;
}
