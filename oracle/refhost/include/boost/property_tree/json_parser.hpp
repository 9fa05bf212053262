// Stand-in for <boost/property_tree/json_parser.hpp>: Cfg::loadConfigFile names read_json, the dumper never calls it
// (its settings come from key=value arguments).  Written for oracle/refhost.py.  TEST INFRASTRUCTURE ONLY.
#pragma once

#include <stdexcept>
#include <string>

#include "ptree.hpp"

namespace boost {
namespace property_tree {
namespace json_parser {

inline void read_json( const std::string&, ptree& ) {
	throw std::runtime_error( "ptree stand-in: read_json is not provided" );
}

}   // namespace json_parser
}   // namespace property_tree
}   // namespace boost
