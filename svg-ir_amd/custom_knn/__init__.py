"""Drop-in replacement of the reference's `custom_knn` package (imported by scene/gaussian_model.py:14; no source upstream):
`custom_knn._C.topKdistCUDA2`."""
