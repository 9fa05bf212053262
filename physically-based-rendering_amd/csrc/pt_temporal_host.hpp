// pt_temporal_host.hpp — the host side of pbr_denoise_temporal's history (pbr_hip.hip) that needs no device: when the history
// is dropped, when a vertex update has to keep the old positions first, and which of the two integration paths a call takes
// (csrc/pt_temporal.hpp).  Host code only, no HIP: tests/temporal_motion_driver.cpp builds it with a plain C++17 compiler.
//
// The history of pbr_denoise_temporal was made under one set of vertex positions, H: those current at the last successful
// call.  Without motion tracking (pbr_temporal_track_motion, off by default) geometry is static: pbr_update_vertices drops the
// history.  With it the history survives an update, and the context keeps H in a second vertex buffer:
//   - the FIRST update after a successful temporal call copies the current vertices there before it overwrites them;
//   - later updates before the next temporal call leave H alone (the history is still the one made under H);
//   - a successful temporal call makes the current vertices H again: `moved` is cleared, nothing is copied.
// A call takes the motion path only if tracking is on, a history is there and the geometry has moved since it was made;
// every other call runs the static kernel, bit for bit what it was before tracking existed.
#pragma once

struct TemporalPolicy {
	bool tracking = false;     // pbr_temporal_track_motion: survives pbr_configure and pbr_upload_scene
	bool history = false;      // the previous successful call's planes are a history
	bool moved = false;        // tracking only: the geometry was updated since the history was made, the second buffer holds H
	bool lastMotion = false;   // the last successful call took the motion path: its motion and face planes can be read

	enum Path { STATIC = 0, MOTION = 1 };

	// pbr_temporal_track_motion( on ).  Turning it off gives the second vertex buffer back (the caller frees it whenever this is
	// called with on == false), and a history whose H is no longer the current geometry goes with it.
	void track( bool on ) {
		if( !on && moved ) {
			history = false;
		}
		if( !on ) {
			moved = false;
		}

		tracking = on;
	}

	// pbr_temporal_reset, pbr_upload_scene, and whatever else invalidates the planes' CONTENT
	void drop() {
		history = false;
		moved = false;
	}

	// pbr_configure: the planes themselves are freed
	void configure() {
		drop();
		lastMotion = false;
	}

	// A pbr_update_vertices that passed its checks.  -> true: copy the current vertices to the second buffer BEFORE they are
	// overwritten.
	bool update() {
		if( !tracking ) {
			drop();
			return false;
		}
		if( !history || moved ) {
			return false;   // nothing to keep positions for, or H is kept already
		}

		moved = true;
		return true;
	}

	// the path of a temporal call that passed its checks
	Path path() const {
		return ( tracking && history && moved ) ? MOTION : STATIC;
	}

	// a temporal call succeeded on `taken`: its planes are the history, made under the current vertices.  (A refused call
	// calls nothing here: it leaves no trace.)
	void succeeded( Path taken ) {
		history = true;
		moved = false;
		lastMotion = ( taken == MOTION );
	}
};
