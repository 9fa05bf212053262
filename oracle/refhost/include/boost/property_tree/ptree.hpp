// Stand-in for <boost/property_tree/ptree.hpp>: a flat map from dotted key to text, which is all the reference's Cfg asks
// of its property tree.  Written for oracle/refhost.py.  TEST INFRASTRUCTURE ONLY.  The driver (dump.cpp) fills it from
// key=value arguments through Cfg::value( key, void* ) -> put( key, void* ): a non-null pointer is taken as a C string
// (only the driver passes one), a null pointer stores "0" (the reference itself switches shadow rays off that way,
// LightParser.cpp's `value( RENDER_SHADOWRAYS, 0 )`).  get<T> converts like Boost's stream translator: numbers through
// operator>>, bool from "true" / "false" / "1" / "0"; a missing key throws.
#pragma once

#include <map>
#include <sstream>
#include <stdexcept>
#include <string>

namespace boost {
namespace property_tree {

class ptree {

	public:
		template<typename T> T get( const char* key ) const {
			std::map<std::string, std::string>::const_iterator it = mValues.find( key );

			if( it == mValues.end() ) {
				throw std::runtime_error( std::string( "ptree stand-in: no such key: " ) + key );
			}

			return convert( it->second, (T*) 0 );
		}

		void put( const char* key, void* value ) {
			mValues[key] = value ? std::string( (const char*) value ) : std::string( "0" );
		}

	private:
		template<typename T> static T convert( const std::string& text, T* ) {
			std::istringstream in( text );
			T v = T();

			if( !( in >> v ) ) {
				throw std::runtime_error( "ptree stand-in: cannot convert \"" + text + "\"" );
			}

			return v;
		}

		static bool convert( const std::string& text, bool* ) {
			if( text == "true" || text == "1" ) { return true; }
			if( text == "false" || text == "0" ) { return false; }
			throw std::runtime_error( "ptree stand-in: not a bool: \"" + text + "\"" );
		}

		static std::string convert( const std::string& text, std::string* ) { return text; }

		std::map<std::string, std::string> mValues;

};

}   // namespace property_tree
}   // namespace boost
