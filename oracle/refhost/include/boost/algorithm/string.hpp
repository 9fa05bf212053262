// Stand-in for <boost/algorithm/string.hpp>: trim, split and is_any_of as the reference's parsers call them, written for
// oracle/refhost.py.  TEST INFRASTRUCTURE ONLY.
//   trim( s )                    removes leading and trailing std::isspace characters, in place
//   split( out, s, is_any_of )   Boost's default, token_compress_off: every separator ends a token, so two adjacent
//                                separators give an empty token and a string without separators gives one token
#pragma once

#include <cctype>
#include <string>
#include <vector>

namespace boost {

struct any_of_pred {
	std::string set;
	bool operator()( char c ) const { return set.find( c ) != std::string::npos; }
};

inline any_of_pred is_any_of( const char* set ) { return any_of_pred { set }; }

template<typename Pred>
inline std::vector<std::string>& split( std::vector<std::string>& out, const std::string& s, Pred isSeparator ) {
	out.clear();
	std::string token;

	for( char c : s ) {
		if( isSeparator( c ) ) {
			out.push_back( token );
			token.clear();
		}
		else {
			token.push_back( c );
		}
	}

	out.push_back( token );
	return out;
}

namespace algorithm {

inline void trim( std::string& s ) {
	size_t b = 0, e = s.size();

	while( b < e && std::isspace( (unsigned char) s[b] ) ) { b++; }
	while( e > b && std::isspace( (unsigned char) s[e - 1] ) ) { e--; }

	s = s.substr( b, e - b );
}

using boost::is_any_of;
using boost::split;

}   // namespace algorithm

using algorithm::trim;

}   // namespace boost
