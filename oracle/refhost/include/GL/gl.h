/* Stand-in for <GL/gl.h>: the OpenCL headers and the reference's parsers include it for its integer type names only.
 * Written for oracle/refhost.py.  TEST INFRASTRUCTURE ONLY. */
#ifndef REFHOST_GL_STANDIN_H
#define REFHOST_GL_STANDIN_H

typedef unsigned int GLenum;
typedef unsigned int GLuint;
typedef int GLint;
typedef int GLsizei;
typedef unsigned int GLbitfield;
typedef float GLfloat;

#endif
