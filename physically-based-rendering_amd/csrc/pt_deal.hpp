// pt_deal.hpp — the dealing orders of the banded work queue (pt_kernel.hpp, nextSlot): the grid the local tiles form, the three
// orders a band's tiles can be dealt in, the rule that picks one by the size of the render call, the check of a table a caller
// hands in (pbr_diag_set_tile_order) and the table of an adaptive round (the active tiles only).  Host code only, no HIP and no
// context: tests/deal_order_driver.cpp and tests/adaptive_driver.cpp build it with a plain C++17 compiler.  `bands` is PT_BANDS
// (pbr_hip.hip passes it); every `first` array holds bands + 1 entries.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "pbr_hip.h"

// The three orders; the values index the context's tables (pbr_hip.hip) and are pbr_diag_get_tile_order's `which`.
enum DealOrder { kDealSpatial = 0, kDealCostClasses = 1, kDealExpensiveLast = 2 };
const int kDealOrders = 3;

// ---- the dealing order of the banded queue (pt_kernel.hpp, nextSlot) -------------------------------------------------
// The local tiles form a rows x width grid (row-major local tile index; its true shape when unsharded, about that
// when sharded).  Band b holds the rows [ b * rows / bands, ( b + 1 ) * rows / bands ); its stretch of the order
// table is [ first[b], first[b + 1] ) and names exactly the band's tiles (the ragged end of the grid is left out).
struct DealGrid { int width = 1, rows = 1; };

// the local tiles as a grid for the banded queue: its true shape when unsharded, about that when sharded
inline DealGrid dealGrid( int tilesX, int numLocalTiles, int tileWorld ) {
	const int width = std::max( 1, ( tilesX + tileWorld - 1 ) / tileWorld );
	return DealGrid{ width, ( numLocalTiles + width - 1 ) / width };
}

// The spatial order (rounds 1 - 5's only one): inside a band column by column, so that the tiles the waves of one XCD hold
// at a time form a compact block of the image, not a strip as wide as the frame.
inline void spatialTileOrder( const DealGrid& grid, int numLocalTiles, int bands, std::vector<unsigned>* order, unsigned* first ) {
	order->clear();
	order->reserve( (size_t) numLocalTiles );

	for( int band = 0; band < bands; band++ ) {
		const unsigned row0 = ( (unsigned) band * (unsigned) grid.rows ) / (unsigned) bands;
		const unsigned rows = ( (unsigned) ( band + 1 ) * (unsigned) grid.rows ) / (unsigned) bands - row0;
		first[band] = (unsigned) order->size();

		for( unsigned col = 0; col < (unsigned) grid.width; col++ ) {
			for( unsigned row = 0; row < rows; row++ ) {
				const unsigned tile = ( row0 + row ) * (unsigned) grid.width + col;

				if( tile < (unsigned) numLocalTiles ) {
					order->push_back( tile );
				}
			}
		}
	}

	first[bands] = (unsigned) order->size();
}

// Cost-ordered dealing.  A launch ends at the pace of its longest paths ("How a launch ends"): when the queue runs
// dry every lane holds a path, and the machine empties while the longest of them finish — 0.5 ms on a Sponza-class scene,
// whatever the launch's length.  Dealt expensive tiles first, the paths that start last are short ones.  Measured (round 6,
// profiles/r06/experiments/deal_order*.txt; round 4 had measured the unsharded half of it, profiles/r04/experiments/
// heaviest_tiles_first.txt): rank 0's share of a 20-frame render split 8 ways -3.5 ... -8 % (Sponza-class 3.14 -> 3.00 ms,
// Dragon-class 3.85 -> 3.72, hairball 6.97 -> 6.72, Cornell 1.50 -> 1.42), its single frame -2 ... -10 %; but a long launch
// LOSES 1 - 8 % because the tiles an XCD holds at one time are no longer neighbours (Sponza-class 64 frames 60.5 -> 61.1 ms,
// hairball 127.9 -> 131.5) and a single full frame neither gains nor loses.  So falling classes only up to kCostOrderTileFrames
// tiles x frames (what is dealt above that: next paragraph).  Eight classes by the band's own cost octiles — the finer the
// classes the less locality is left, a full sort is the worst on long launches and no better on short.
//
// LONG launches (found late in round 6, profiles/r06/experiments/deal_order_ascending*.txt, band_balance*.txt): the same cost
// map, the other way round.  A band that deals its most EXPENSIVE quarter LAST — spatial order inside both parts — renders a long
// launch 1 - 7 % faster than the spatial order: Sponza-class 20 frames 19.37 -> 19.10 ms (two-paths plan), 20.13 -> 19.60 (6 waves);
// Dragon-class 19.85 -> 18.60 ms, 64 frames 61.1 -> 57.0; hairball 127.7 -> 125.2; Cornell 27.2 -> 26.1; the eight-order walk alike
// (Dragon-class 49.96 -> 47.14 ms); rank 0 of 8 from ~40 frames on.  The gain is proportional to the launch's length, the opposite
// direction (expensive first) loses as much, the split point hardly matters (15 / 25 / 40 %), ascending classes do the same and
// interleaving the classes does not: what counts is that a band's heavy tiles come when the XCDs whose own bands are cheap have
// run out of them and join in (bands differ by up to 10 x in cost, and an XCD works on its own band until it is empty) — the
// heavy part of every band is then shared by all eight XCDs, their L2s and their fabric links, instead of being its owner's alone.
// Equalising the bands' costs by moving their row boundaries gives a fifth of that; and the heavy tiles have to be the VERY last a
// band deals: a coda of its cheapest 10 % behind them gives the whole gain back (band_balance_cheap_coda.txt).  That was the clue:
// most of it was the QUEUE HEADS.  The XCDs that have run dry all draw from the one head of the band they help, a head hands out
// ~90 draws / us, and cheap tiles are drawn the fastest — expensive-last merely made sure that the shared part of a launch draws
// slowly.  With four heads per band and the helpers spread over them (pt_kernel.hpp, nextSlot; experiments/queue_heads_*.txt,
// queue_subheads_*.txt) the SPATIAL order is as fast as expensive-last was (Sponza-class 64 frames 2165 -> 2211 Msamples/s against
// 2196; Dragon-class 2132 -> 2317 against 2290; Cornell 4832 -> 5148 against 5053) and expensive-last still adds 1.3 % on the
// Dragon-class scene and Cornell, nothing on the other two.  Below ~192 Ki tiles x frames it loses to the
// spatial order (the long paths start last), hence three orders by the size of the RENDER CALL (all launches of a call alike;
// while the schedule tuner is still measuring, everything is dealt spatially: dealRule):
//   tiles x frames <= 128 Ki  eight classes of falling cost     <= 192 Ki  spatial     above  expensive quarter last
// A SHARD (tile_world > 1) deals falling classes up to 1 Mi tiles x frames: its tiles are every N-th of the image, the spatial order
// has little locality to lose there, and with the heads out of the way the shorter end is what is left to gain — rank 0's share at
// 20 frames, N = 2 / 4: Sponza-class 10.24 -> 10.07 ms, 5.54 -> 5.40; Dragon-class 10.67 -> 10.58, 6.23 -> 6.09; N = 8 at 64 frames
// 8.29 -> 8.13, 8.97 -> 8.80 (queue_subheads_orders_by_launch_length.txt).  Small UNSHARDED images do not share that: 1280x720 ...
// 640x360 behave like 1080p (queue_subheads_orders_small_and_4k_images.txt).
const unsigned kCostClasses = 8;
const size_t kCostOrderTileFrames = 128 * 1024;
const size_t kCostOrderShardTileFrames = 1024 * 1024;
const size_t kSpatialOrderTileFrames = 192 * 1024;

// The dealing order of a render call of `tiles` local tiles x `frames` frames, by its size.  Spatial while the order is pinned
// (pbr_diag_set_tile_order), no costs have been learnt or the deal_order knob is 0; a knob of 1 or 2 forces that order.  Until
// the schedule tuner has settled (or the plan is fixed: a pinned plan, Phong tessellation, an adaptive render), everything is
// dealt spatially: its chunks are short launches whatever the call's length, the cost orders are made for one length each
// (expensive-last costs a 2-frame launch 6 %), and a plan's fitted fixed cost must not depend on which of them its chunks
// happened to run in (seen: the 6-waves plan kept over the two-paths one, -3.6 %).
inline DealOrder dealRule( bool pinned, bool learnt, int knob, bool settled, bool sharded, size_t tiles, size_t frames ) {
	if( pinned || !learnt || knob == 0 || !( settled || knob > 0 ) ) {
		return kDealSpatial;
	}

	const size_t tileFrames = tiles * frames;
	const size_t costLimit = sharded ? kCostOrderShardTileFrames : kCostOrderTileFrames;
	return ( knob > 0 ) ? ( knob == 1 ? kDealCostClasses : kDealExpensiveLast )
	       : ( tileFrames <= costLimit ) ? kDealCostClasses : ( tileFrames <= kSpatialOrderTileFrames ) ? kDealSpatial : kDealExpensiveLast;
}

// what pbr_diag_last_deal calls a render dealt in `dealt` (a pinned table sits in the spatial order's place)
inline const char* dealName( bool pinned, DealOrder dealt ) {
	const char* const names[kDealOrders] = { "spatial", "cost-classes", "expensive-last" };
	return pinned ? "pinned" : names[dealt];
}

// per band: the spatial order, stably partitioned into [ the cheaper three quarters ][ the most expensive quarter ]
inline void expensiveLastTileOrder( const unsigned* bandFirst, int bands, const std::vector<unsigned>& spatial, const std::vector<float>& cost, std::vector<unsigned>* order ) {
	order->assign( spatial.size(), 0u );
	std::vector<float> sorted;

	for( int band = 0; band < bands; band++ ) {
		const unsigned first = bandFirst[band], n = bandFirst[band + 1] - first;

		if( n == 0 ) {
			continue;
		}

		sorted.resize( n );

		for( unsigned k = 0; k < n; k++ ) {
			sorted[k] = cost[spatial[first + k]];
		}

		std::sort( sorted.begin(), sorted.end() );
		const float edge = sorted[std::min<size_t>( n - 1, ( (size_t) 3 * n ) / 4 )];
		unsigned at = first;

		for( int pass = 0; pass < 2; pass++ ) {
			for( unsigned k = 0; k < n; k++ ) {
				const unsigned tile = spatial[first + k];

				if( ( cost[tile] > edge ) == ( pass == 1 ) ) {
					( *order )[at++] = tile;
				}
			}
		}
	}
}

// per band: the spatial order, stably partitioned into kCostClasses classes of falling cost (class edges = the band's octiles)
inline void costTileOrder( const unsigned* bandFirst, int bands, const std::vector<unsigned>& spatial, const std::vector<float>& cost, std::vector<unsigned>* order ) {
	order->assign( spatial.size(), 0u );
	std::vector<float> sorted;
	std::vector<unsigned> fill( kCostClasses );

	for( int band = 0; band < bands; band++ ) {
		const unsigned first = bandFirst[band], n = bandFirst[band + 1] - first;

		if( n == 0 ) {
			continue;
		}

		sorted.resize( n );

		for( unsigned k = 0; k < n; k++ ) {
			sorted[k] = cost[spatial[first + k]];
		}

		std::sort( sorted.begin(), sorted.end() );
		float edge[kCostClasses - 1];

		for( unsigned c = 0; c + 1 < kCostClasses; c++ ) {
			edge[c] = sorted[std::min<size_t>( n - 1, ( (size_t) ( c + 1 ) * n ) / kCostClasses )];
		}

		// class 0 = the most expensive: a tile's class counts the edges its cost stays below
		auto classOf = [&]( float v ) {
			unsigned below = 0;

			for( unsigned c = 0; c + 1 < kCostClasses; c++ ) {
				below += ( v < edge[c] ) ? 1u : 0u;
			}

			return below;
		};

		std::fill( fill.begin(), fill.end(), 0u );

		for( unsigned k = 0; k < n; k++ ) {
			fill[classOf( cost[spatial[first + k]] )]++;
		}

		unsigned at = 0;

		for( unsigned c = 0; c < kCostClasses; c++ ) {
			const unsigned size = fill[c];
			fill[c] = at;
			at += size;
		}

		for( unsigned k = 0; k < n; k++ ) {
			const unsigned tile = spatial[first + k];
			( *order )[first + fill[classOf( cost[tile] )]++] = tile;
		}
	}
}

// Why pbr_diag_set_tile_order refuses this table of `count` entries (PBR_EINVAL, the message in *why), or PBR_OK.  spatial /
// spatialFirst: the spatial order of the queue's grid.  band_first (bands + 1 entries) may be null: the bands are the spatial ones.
inline int tileOrderCheck( const uint32_t* order, uint32_t count, const uint32_t* band_first, const std::vector<unsigned>& spatial,
                           const unsigned* spatialFirst, int bands, std::string* why ) {
	char buf[256];

	if( count != (uint32_t) spatial.size() ) {
		std::snprintf( buf, sizeof( buf ), "diag_set_tile_order: %u entries, the queue has %zu tiles", count, spatial.size() );
		*why = buf;
		return PBR_EINVAL;
	}

	const uint32_t* first = ( band_first != nullptr ) ? band_first : spatialFirst;

	if( first[0] != 0u || first[bands] != count ) {
		std::snprintf( buf, sizeof( buf ), "diag_set_tile_order: the bands' stretches must cover the table: band_first[0] = 0, band_first[%d] = %u", bands, count );
		*why = buf;
		return PBR_EINVAL;
	}

	for( int band = 0; band < bands; band++ ) {
		if( first[band] > first[band + 1] ) {
			std::snprintf( buf, sizeof( buf ), "diag_set_tile_order: band_first must not decrease (band %d)", band );
			*why = buf;
			return PBR_EINVAL;
		}
	}

	// the table must name every local tile exactly once: a unit dealt twice or never is a wrong image.  Without band_first the
	// bands are the spatial ones and every band's stretch must hold that band's own tiles.
	std::vector<unsigned char> bandOf( spatial.size(), 1 );

	if( band_first == nullptr ) {
		for( int band = 0; band < bands; band++ ) {
			for( unsigned k = spatialFirst[band]; k < spatialFirst[band + 1]; k++ ) {
				bandOf[spatial[k]] = (unsigned char) ( band + 1 );
			}
		}
	}

	for( int band = 0; band < bands; band++ ) {
		for( unsigned k = first[band]; k < first[band + 1]; k++ ) {
			const uint32_t tile = order[k];
			const unsigned char want = ( band_first == nullptr ) ? (unsigned char) ( band + 1 ) : (unsigned char) 1;

			if( tile >= (uint32_t) bandOf.size() || bandOf[tile] != want ) {
				std::snprintf( buf, sizeof( buf ), "diag_set_tile_order: entry %u (tile %u) is not a tile of band %d, or is named twice", k, tile, band );
				*why = buf;
				return PBR_EINVAL;
			}

			bandOf[tile] = 0;
		}
	}

	return PBR_OK;
}

// A dealing table (band b's stretch is order[ bandFirst[b] .. bandFirst[b + 1] )) without the tiles whose active[tile] is 0
// (pbr_render_adaptive: a round deals the tiles that have not stopped): every band keeps its surviving tiles in the order they
// had; a band may come out empty (two equal bandFirst entries — nextSlot takes a band of 0 tiles as exhausted).
inline void filterOrder( const std::vector<unsigned>& order, const unsigned* bandFirst, const unsigned* active, int bands,
                         std::vector<unsigned>* out, unsigned* outFirst ) {
	out->clear();

	for( int band = 0; band < bands; band++ ) {
		outFirst[band] = (unsigned) out->size();

		for( unsigned k = bandFirst[band]; k < bandFirst[band + 1]; k++ ) {
			if( active[order[k]] != 0u ) {
				out->push_back( order[k] );
			}
		}
	}

	outFirst[bands] = (unsigned) out->size();
}
