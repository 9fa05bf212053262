// Stand-in for <boost/date_time/posix_time/posix_time.hpp>: the reference only times its own steps for log lines.
// Written for oracle/refhost.py.  TEST INFRASTRUCTURE ONLY.  Every clock reads zero, so nothing a run prints or writes
// depends on the time.
#pragma once

namespace boost {
namespace posix_time {

struct time_duration {
	long total_milliseconds() const { return 0; }
};

struct ptime {};

inline time_duration operator-( const ptime&, const ptime& ) { return time_duration(); }

struct microsec_clock {
	static ptime local_time() { return ptime(); }
};

}   // namespace posix_time
}   // namespace boost
