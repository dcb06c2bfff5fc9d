/* The three CPython 3.13 functions the reference's glue takes from its `pythoncapi-compat` submodule (empty in the
 * snapshot, R:scs/scsobject.h:1,112,154,168), backported for older interpreters.  Found by oracle/ref_glue.py through
 * -idirafter, so a real copy of the submodule would win. */
#include <Python.h>
#if PY_VERSION_HEX < 0x030D0000
static inline int PyDict_GetItemStringRef(PyObject *d, const char *k, PyObject **out) {
  PyObject *key = PyUnicode_FromString(k);
  if (!key) { *out = NULL; return -1; }
  PyObject *v = PyDict_GetItemWithError(d, key);
  Py_DECREF(key);
  if (v) { Py_INCREF(v); *out = v; return 1; }
  *out = NULL;
  return PyErr_Occurred() ? -1 : 0;
}
static inline PyObject *PyList_GetItemRef(PyObject *l, Py_ssize_t i) {
  PyObject *v = PyList_GetItem(l, i);
  Py_XINCREF(v);
  return v;
}
#endif
