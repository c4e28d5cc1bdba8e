function I = local_cn(I)
% Local contrast normalisation of images or video frames on the GPU: the function
% 3D/extractContrastNormalizatonMovie.m:30 calls and the reference does not ship.
% I: [H, W] or [H, W, n], any numeric class, any size H, W >= 7.  Each frame gets
% CreateImages' 'local_cn' (image_helpers/CreateImages.m:299-369: 13x13 Gaussian of
% sigma 3*1.591, rconv2 reflection, std floored at its median) followed by ZERO_MEAN
% (CreateImages.m:652-657), and comes back as single, as CreateImages stores it.
% Runs on the first GPU of ccsc_device() through ccsc_localcn_mex (libccsc's
% ccsc_local_cn).
    I = single(ccsc_localcn_mex(double(I), ccsc_device()));
end
