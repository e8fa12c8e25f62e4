/* Stand-in for <GL/glew.h>, used only by oracle/ref_build.py when it compiles the reference's src/cprocess where it lies.
 * The reference's CPU pixel code never calls GL; its GL halves only have to compile.  The system's own GL headers declare
 * the entry points (their definitions stay unresolved in the library, which is loaded with lazy binding), and the one GLEW
 * type that framework.h names is left opaque. */
#ifndef CANVAS_REF_SHIM_GLEW_H
#define CANVAS_REF_SHIM_GLEW_H
#define GL_GLEXT_PROTOTYPES 1
#include <GL/gl.h>
#include <GL/glext.h>
typedef struct GLEWContextStruct GLEWContext;
#endif
