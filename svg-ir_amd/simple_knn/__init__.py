"""Drop-in replacement of the reference's `simple_knn` package (submodules/simple-knn): `simple_knn._C.distCUDA2`."""
