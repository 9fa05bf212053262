// pt_tuner.hpp — the schedule tuner of launch() (pbr_hip.hip): which of the kPlans plans renders each chunk of a render call.
// Host code only, no HIP: tests/schedule_tuner_driver.cpp builds it with a plain C++17 compiler and drives it with synthetic
// timings.  The library's host code is built with -ffp-contract=off; so is the driver, so that the fits come out the same.
//
// Which kernel: the lock-step walk ("refill") or the lane state machine ("phased"), each with the lean (4 waves / SIMD, no
// spills), the mid (6) or the wide (8 waves / SIMD) register budget.  Which one wins depends on the scene (1080p: Cornell
// refill-mid 4250 vs phased-mid 3650 Msamples/s, dragon-class phased-mid 1900 vs refill-wide 1000), and all of them give the
// same bits — so the first frames of a scene + configuration, which have to be rendered anyway, are rendered in turn by each
// candidate (kScreenFrames each) and timed; short launches favour the plans with fewer, larger blocks, so the two or three
// fastest (the third only if within 10 % of the first) are timed again on short and long chunks, in the palindromic order
// A B C (short) C B A (long) A B C (long) C B A (short): two lengths separate a launch's fixed cost from its per-frame cost, and
// every plan's short launches and its long launches are centred on the same moment, so the drift of the clocks — the GPU ramps
// up from idle during exactly these launches, which biased a one-sided order by 5 % in the per-frame cost — cancels in both.
// When the two best end within 5 % of each other the palindrome is run a second time before the decision (the fits
// accumulate): a fit over four launches carries 1 - 5 % of noise.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

// One chunk of a render call: the plan that renders it and how many frames.
struct Chunk {
	int plan;
	uint32_t frames;
	int finalist;      // refinement: index into the finalists; < 0 otherwise
	bool screening;
};

class ScheduleTuner {
public:
	static constexpr int kPlans = 7;

	// Lengths in 1080p-frame equivalents: a rank of an 8-GPU run (or a small image) has 1/8 of the pixels per frame, and
	// launches of a few hundred microseconds say little about a long render (measured at 1/8 of the tiles: the tuner kept a
	// plan 26 % slower than the best).  So the chunk lengths grow as the frame shrinks: the scale is how many frames of
	// `localPixels` pixels make one 1080p frame.
	static uint32_t scaleOf( size_t localPixels ) {
		const size_t reference = (size_t) 1920 * 1080;
		const size_t scale = ( reference + localPixels / 2 ) / std::max<size_t>( localPixels, 1 );
		return (uint32_t) std::min<size_t>( std::max<size_t>( scale, 1 ), 64 );
	}

	// tune_log: the [pbr tune] lines go to `log` (nullptr: none), naming the plans by `names`
	FILE* log = nullptr;
	const char* names[kPlans] = {};

	// Starts over (a new scene, a new configuration, a changed knob), at the scale of the configuration.
	void reset( uint32_t scale ) {
		scale_ = scale;
		tuned_ = -1;
		renderFrames_ = tunedAt_ = 0;
		std::memset( screen_, 0, sizeof( screen_ ) );
		finalists_ = 0;
		restartRefinement();
	}

	// A render call of nFrames frames begins.
	void beginRender( uint32_t nFrames ) {
		renderFrames_ = std::max( renderFrames_, nFrames );

		if( tuned_ >= 0 && finalists_ > 0 && nFrames > kReevaluateRatio * tunedAt_ ) {
			// tuned for shorter renders than this one (a viewer's frame-by-frame calls, then a batch): the fixed cost
			// weighs less now.  With fits from two launch lengths that is a new evaluation; with one length only, the
			// finalists are timed again on this render's frames.
			const Decision again = decide( nFrames );

			if( again.separable ) {
				tuned_ = again.plan;
				tunedAt_ = nFrames;
			}
			else if( nFrames >= kRetimeLongChunks * refineLong() ) {
				tuned_ = -1;
				restartRefinement();
			}
		}
	}

	bool settled() const { return tuned_ >= 0; }
	int tunedPlan() const { return tuned_; }

	// Which plan renders the next chunk, and how many of the (at most) maxFrames frames the call has left for it.
	Chunk next( uint32_t maxFrames ) const {
		if( tuned_ >= 0 ) {
			return Chunk{ tuned_, maxFrames, -1, false };
		}

		if( finalists_ > 0 ) {
			// forward, then backward (A B C C B A): symmetric against a clock that is still ramping up or throttling
			const uint32_t k = refineChunks_ % (uint32_t) finalists_;
			const uint32_t pass = refineChunks_ / (uint32_t) finalists_;
			const int finalist = ( ( pass & 1u ) != 0u ) ? finalists_ - 1 - (int) k : (int) k;
			const bool longPass = ( pass % kRefinePasses == 1u || pass % kRefinePasses == 2u );
			return Chunk{ finalist_[finalist], std::min<uint32_t>( maxFrames, longPass ? refineLong() : refineShort() ), finalist, false };
		}

		int plan = 0;

		while( plan < kPlans - 1 && screened( plan ) ) {
			plan++;
		}

		return Chunk{ plan, std::min<uint32_t>( maxFrames, screenFrames() - screen_[plan].frames ), -1, true };
	}

	// What a chunk took, in ms; chunks that measure nothing (a settled tuner's) are ignored.
	void record( const Chunk& c, double ms ) {
		if( !c.screening && c.finalist < 0 ) {
			return;
		}

		const uint32_t n = c.frames;

		if( log != nullptr ) {
			std::fprintf( log, "[pbr tune] %s %-12s %u frame(s) %.3f ms = %.3f ms/frame\n", c.screening ? "screen" : "refine", names[c.plan], n, ms, ms / n );
		}

		if( c.screening ) {
			screen_[c.plan].ms += ms;
			screen_[c.plan].frames += n;
			screen_[c.plan].launches++;

			if( screened( kPlans - 1 ) ) {
				chooseFinalists();
			}

			return;
		}

		double* fit = fit_[c.finalist];
		fit[0] += 1.0;
		fit[1] += (double) n;
		fit[2] += (double) n * (double) n;
		fit[3] += ms;
		fit[4] += (double) n * ms;
		refineChunks_++;

		if( refineChunks_ >= rounds_ * kRefinePasses * (uint32_t) finalists_ ) {
			const Decision best = decide( renderFrames_ );

			// A close call — the runner-up within 5 % (phased-mid and phased-dual on a Sponza-class scene are 3 % apart, and a
			// fit over four launches per plan carries 1 - 5 % of noise in its per-frame cost: measured, one wrong pick in a dozen
			// runs) — gets a second palindrome of launches before the decision; the fits accumulate.
			if( best.runnerUp > 0.0 && best.runnerUp < kCloseCall && rounds_ < kMaxRounds ) {
				rounds_ = kMaxRounds;
			}
			else {
				tuned_ = best.plan;
				tunedAt_ = renderFrames_;
			}
		}
	}

	// The fit of `plan`'s refinement launches, a + b x frames in ms: only a proper one (two lengths, a >= 0, b >= 0).
	bool fit( int plan, double* a, double* b ) const {
		for( int k = 0; k < finalists_; k++ ) {
			double aFit, bFit;

			if( finalist_[k] == plan && solve( fit_[k], &aFit, &bFit ) && aFit >= 0.0 && bFit >= 0.0 ) {
				*a = aFit;
				*b = bFit;
				return true;
			}
		}

		return false;
	}

	// The frames the tuner renders before it settles, at most: every plan screened, then the most finalists over both rounds
	// of the palindrome (each finalist: kRefinePasses / 2 short and as many long chunks per round).
	uint32_t budgetFrames() const {
		return (uint32_t) kPlans * screenFrames() + kMaxRounds * (uint32_t) kMaxFinalists * ( kRefinePasses / 2u ) * ( refineShort() + refineLong() );
	}

private:
	// screening: kScreenFrames frames per plan, or kScreenLaunches launches, whichever comes first
	static constexpr uint32_t kScreenFrames = 2, kScreenLaunches = 2;
	// refinement: every plan within 10 % of the fastest (at least the two fastest, at most three) goes on to it
	static constexpr int kMinFinalists = 2, kMaxFinalists = 3;
	static constexpr double kFinalistMargin = 1.10;
	// ... on chunks of two lengths, over kRefinePasses passes: short, long, long, short
	static constexpr uint32_t kRefineShort = 4, kRefineLong = 12, kRefinePasses = 4;
	// a close call (the best two within 5 %) gets a second round
	static constexpr double kCloseCall = 1.05;
	static constexpr uint32_t kMaxRounds = 2;
	// a render longer than twice the one the plan was chosen for is evaluated again; without separable fits the finalists
	// are timed again on it if it holds kRetimeLongChunks long chunks
	static constexpr uint32_t kReevaluateRatio = 2, kRetimeLongChunks = 4;

	uint32_t screenFrames() const { return kScreenFrames * scale_; }
	uint32_t refineShort() const { return kRefineShort * scale_; }
	uint32_t refineLong() const { return kRefineLong * scale_; }

	bool screened( int plan ) const {
		return screen_[plan].frames >= screenFrames() || screen_[plan].launches >= kScreenLaunches;
	}

	void restartRefinement() {
		refineChunks_ = 0;
		rounds_ = 1;
		std::memset( fit_, 0, sizeof( fit_ ) );
	}

	void chooseFinalists() {
		auto perFrame = [&]( int k ) { return screen_[k].ms / screen_[k].frames; };
		int order[kPlans] = { 0, 1, 2, 3, 4, 5, 6 };
		std::sort( order, order + kPlans, [&]( int x, int y ) { return perFrame( x ) < perFrame( y ); } );
		finalists_ = 0;

		for( int k = 0; k < kPlans; k++ ) {
			if( k < kMinFinalists || ( k < kMaxFinalists && perFrame( order[k] ) <= kFinalistMargin * perFrame( order[0] ) ) ) {
				finalist_[finalists_++] = order[k];
			}
		}
	}

	// Least squares of a + b x n over the sums f (false: singular — launches of one length only).
	static bool solve( const double f[5], double* a, double* b ) {
		const double det = f[0] * f[2] - f[1] * f[1];

		if( !( det > 1e-9 * f[2] * f[0] ) ) {
			return false;
		}

		*b = ( f[0] * f[4] - f[1] * f[3] ) / det;
		*a = ( f[3] - *b * f[1] ) / f[0];
		return true;
	}

	// A launch costs a + b x frames (a: ramp-up and drain, 0.3 - 0.6 ms; b: the per-frame rate) and the plans differ in both:
	// least squares over each finalist's refinement launches, then the cost of a render of `renderFrames` frames.  Launches of
	// one length only (a caller rendering frame by frame) cannot separate the two: a = 0, separable false.  runnerUp: the
	// cost of the second-best finalist relative to the best's.
	struct Decision { int plan; bool separable; double runnerUp; };
	Decision decide( uint32_t renderFrames ) const {
		const double frames = (double) std::max<uint32_t>( renderFrames, 1u );
		int best = -1;
		double bestCost = 0.0, secondCost = 0.0;
		bool separable = true;

		for( int k = 0; k < finalists_; k++ ) {
			const double* f = fit_[k];
			double a = 0.0, b = f[3] / f[1], aFit, bFit;
			const bool solved = solve( f, &aFit, &bFit );
			separable = separable && solved;

			if( solved && aFit >= 0.0 && bFit >= 0.0 ) {   // else the mean over the launches, without a fixed cost
				a = aFit;
				b = bFit;
			}

			const double cost = ( a + b * frames ) / frames;

			if( log != nullptr ) {
				std::fprintf( log, "[pbr tune] fit %-12s a %.3f ms  b %.3f ms/frame  -> %.4f ms/frame at %u frames\n", names[finalist_[k]], a, b, cost, (unsigned) frames );
			}

			if( best < 0 || cost < bestCost ) {
				secondCost = ( best < 0 ) ? 0.0 : bestCost;
				best = k;
				bestCost = cost;
			}
			else if( secondCost == 0.0 || cost < secondCost ) {
				secondCost = cost;
			}
		}

		return Decision{ finalist_[best], separable, ( bestCost > 0.0 && secondCost > 0.0 ) ? secondCost / bestCost : 0.0 };
	}

	uint32_t scale_ = 1;
	int tuned_ = -1;                       // the plan kept; -1 while measuring
	uint32_t renderFrames_ = 0;            // the longest render (frames per call) asked for since the reset
	uint32_t tunedAt_ = 0;                 // the render length tuned_ was chosen for
	struct { double ms; uint32_t frames, launches; } screen_[kPlans] = {};   // screening, per plan
	int finalists_ = 0;                    // refinement: the plans that go on to it, fastest screened first
	int finalist_[kMaxFinalists] = {};
	uint32_t refineChunks_ = 0;            // chunks rendered so far in the refinement
	uint32_t rounds_ = 1;                  // 1; kMaxRounds once a close call has been given a second palindrome
	double fit_[kMaxFinalists][5] = {};    // per finalist, over its refinement launches: sums of 1, n, n^2, ms, n * ms (n = frames of the launch)
};
